// ctgcn_gat.hip — the graph-attention step of the GAT baseline (reference baseline/gat.py:65-105) on the GPU.
//
// One layer has `heads` heads of width F over S [n, d], d = heads F, columns [hF, (h+1)F) holding x W_h.  For a stored entry (i, j):
//   z_ij = u_i + v_j (u = a_src_h · S_i^h, v = a_dst_h · S_j^h), l_ij = -leakyrelu_alpha(z_ij), e_ij = exp(l_ij - m_i), Z_i = sum_j e_ij,
//   Y_i^h = (sum_j q_ij e_ij S_j^h) / Z_i,  q_ij = keep(key + h, i, j) / (1 - p_att)  (1 without attention dropout).
// m_i = max_j l_ij comes from a scalar pre-pass: -leakyrelu is decreasing, so m_i = -leakyrelu(u_i + min_j v_j).  With m known before
// the gather no accumulator is ever rescaled and the pieces of a long row add up like any other sum.
//
// Every gather (forward, and the backward's pass over the CSR and over its transpose) is the pull form of ctgcn_gather.h with the
// entry's weight computed on the fly: LPR lanes own a destination row and a float4 (or a float) per lane of it, entries are read LPR
// at a time and handed round by shuffles, U gathered rows in flight, rows longer than long_threshold go to piece blocks and a
// finishing kernel.  A lane works for the head its columns lie in; F % 4 == 0 on the float4 path, so a float4 never straddles heads.
//
//   backward, for G = d loss / d Y:  D_i = G_i^h · Y_i^h,  p_ij = e_ij / Z_i,  s_ij = (z_ij > 0 ? 1 : alpha),  w_ij = q_ij p_ij
//     row pass   R_i^h = sum_j s_ij w_ij S_j^h,  c_i = sum_j s_ij p_ij          du_i = D_i c_i - G_i^h · R_i^h
//     col pass   A_j^h = sum_i w_ij G_i^h,  B_j^h = sum_i s_ij w_ij G_i^h,  k_j = sum_i s_ij p_ij D_i     dv_j = k_j - S_j^h · B_j^h
//                dS_j^h = A_j^h + du_j a_src_h + dv_j a_dst_h
//     da_src_h = sum_i du_i S_i^h, da_dst_h = sum_i dv_i S_i^h: blockwise column sums from one read of S, added in block order
// which is dl_ij = p_ij (q_ij t_ij - D_i), dz_ij = -s_ij dl_ij with the dot product t_ij = G_i^h · S_j^h moved out of the per-entry
// work: the sums over entries are linear in it, so one dot product per (row, head) on the finished sums replaces one per entry.
// No atomics; every sum has a fixed order, so repeated launches are bit-identical.  Nothing of nnz x F elements exists, and no
// per-entry array at all: p_ij and the dropout draw are recomputed from u, v, m, Z and (key + h, i, j) in each pass.
//
// The same passes serve PyG's GATConv (ctgcn_tgat_*; TgGAT in ctgcn_amd/baseline/tg.py) with lsign = +1: l_ij = +leakyrelu(z_ij), so
// m_i = leakyrelu(u_i + max_j v_j), dz_ij = +s_ij dl_ij and du, dv change sign; the forward adds a bias and its epilogue is ReLU and
// dropout; there is no attention dropout.  With lsign = -1 every expression below reduces to the reference form's bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr int U = 4;                   // gathered rows in flight per lane group
constexpr int FWD = 0, ROW = 1, COL = 2;
constexpr int EPI_NONE = 0, EPI_ELU = 1, EPI_ELU_DROP = 2;
constexpr int EPI_RELU = 3;               // the PyG form's ReLU and dropout (ctgcn_tgat_fwd_f32 alone; the reference-form entry points refuse it)
constexpr int MIN_LANES = 16;          // lanes per row of the row-maximum pre-pass

struct GatArgs {
    int64_t n;
    int32_t d, heads, F;
    const int32_t *row_ptr;
    const int32_t *col;
    const float *src;       // the gathered rows: S (FWD, ROW) or G (COL)
    int64_t ldsrc;
    const float *u;         // FWD: [n, heads]
    const float *v;         // [n, heads]: of the gathered row (FWD, ROW), of the own row (COL)
    const float *m;         // FWD: [n, heads]
    const f4 *pack;         // ROW: of the own row, COL: of the gathered row: {u, m, 1 / Z (0 for an empty row), D} [n, heads]
    const float *ctr;       // ROW, PyG form: Y [n, d], the row's own output, taken off every gathered row (see add_entry); else null
    int64_t ldctr;
    float alpha;
    float lsign;            // l = lsign leakyrelu(z): -1 the reference's layer, +1 PyG's GATConv
    int32_t drop;           // p_att > 0
    double p_att;
    float att_scale;        // 1 / (1 - p_att)
    uint64_t key;
    float *out1;            // FWD: epi(Y); ROW: R; COL: A (null: not wanted)
    int64_t ld1;
    float *out2;            // FWD: Y before the epilogue (null without one); COL: B
    int64_t ld2;
    float *sout;            // [n, heads]  FWD: Z; ROW: c; COL: k
    const float *bias;      // FWD, PyG form: [d] added to Y before the epilogue, or null
    int32_t epi, fdrop;     // FWD: the epilogue; p_feat > 0
    double p_feat;
    float fscale;
    uint64_t fkey;
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t chunks;         // ceil(d / VEC)
    int32_t max_pieces;
    int32_t part_ld;        // d rounded up to 4
    int32_t piece_ld;       // floats per piece: [part_ld] first sum, [part_ld] second sum, [heads rounded up to 4] scalar sums
    float *part;            // [n_long][max_pieces][piece_ld]
};

// what a lane keeps of its own row for the head it works on
struct Own {
    float a;                // u_i (FWD, ROW) or v_j (COL)
    float m, iz;            // FWD: m_i; ROW: m_i, 1 / Z_i
    float s0;               // ROW: a slope taken off every s_ij of the row (see add_entry); 0 in the reference form
    uint64_t key;           // key + h
};

template <int MODE>
__device__ __forceinline__ Own own_of(const GatArgs &a, int64_t row, int h)
{
    Own o;
    const int64_t k = row * a.heads + h;
    o.s0 = 0.f;
    if (MODE == FWD) { o.a = a.u[k]; o.m = a.m[k]; o.iz = 0.f; }
    else if (MODE == ROW) {
        const f4 p = a.pack[k];
        o.a = p.x; o.m = p.y; o.iz = p.z;
        if (a.lsign > 0.f) o.s0 = p.y > 0.f ? 1.f : a.alpha;       // PyG form: the slope at the row's largest logit (m = leakyrelu(z_max))
    }
    else { o.a = a.v[k]; o.m = 0.f; o.iz = 0.f; }
    o.key = a.key + (uint64_t)h;
    return o;
}

// the scalar(s) a lane reads of a gathered row c: v_c (FWD, ROW) or the pack of c (COL)
template <int MODE>
__device__ __forceinline__ f4 side_of(const GatArgs &a, int64_t c, int h)
{
    if (MODE == COL) return a.pack[c * a.heads + h];
    return f4{a.v[c * a.heads + h], 0.f, 0.f, 0.f};
}

// one entry into the sums: (row, c) is the stored entry (i, j) in FWD and ROW, (j, i) in COL
template <int MODE, typename V>
__device__ __forceinline__ void add_entry(const GatArgs &a, const Own &o, int64_t row, int64_t c, f4 side, V x, V &A1, V &A2, float &s)
{
    const float z = MODE == COL ? side.x + o.a : o.a + side.x;
    const bool pos = z > 0.f;
    const float l = a.lsign * (pos ? z : a.alpha * z);
    float q = 1.f;
    if (a.drop) {
        const double r = MODE == COL ? ctgcn_u01(o.key, (uint64_t)c, (uint64_t)row) : ctgcn_u01(o.key, (uint64_t)row, (uint64_t)c);
        q = r >= a.p_att ? a.att_scale : 0.f;
    }
    if (MODE == FWD) {
        const float e = expf(l - o.m);
        s += e;
        A1 = vfma(q * e, x, A1);
    } else if (MODE == ROW) {
        // du_i = sum_j s_ij p_ij (t_ij - D_i) and sum_j p_ij (t_ij - D_i) = 0: any slope s0 constant over the row may be taken off
        // s_ij.  With s0 the slope at the largest logit, a row whose logits lie on one side of 0 gives du_i = 0 exactly, where
        // G·R - D c would leave the rounding of two equal sums (all of att_r's gradient when every row is like that).
        // With a.ctr, A2 holds Y_i and R_i = sum_j w_ij (S_j - Y_i): t_ij - D_i = G_i · (S_j - Y_i) without attention dropout, so
        // du_i = G_i · R_i with c_i left at 0, and what the S_j have in common (a bias of the layer before) never enters the sum.
        const float sp = ((pos ? 1.f : a.alpha) - o.s0) * (expf(l - o.m) * o.iz);
        if (!a.ctr) s += sp;
        A1 = vfma(sp * q, x - A2, A1);                            // A2 = 0 in the reference form
    } else {
        const float p = expf(l - side.y) * side.z;
        const float sl = pos ? 1.f : a.alpha;
        const float w = q * p;
        s = fmaf(sl * p, side.w, s);
        A1 = vfma(w, x, A1);
        A2 = vfma(sl * w, x, A2);
    }
}

// the sums over the entries [start, end) of a row by the row's LPR lanes
template <int VEC, int LPR, int MODE>
__device__ __forceinline__ void row_sum(const GatArgs &a, const Own &o, int64_t row, int h, int start, int end, int lig, int64_t foff,
                                        typename vec_of<VEC>::type &A1, typename vec_of<VEC>::type &A2, float &s)
{
    using V = typename vec_of<VEC>::type;
    for (int base = start; base < end; base += LPR) {
        const int my = base + lig;
        int c = 0;
        if (my < end) c = a.col[my];
        const int cnt = min(LPR, end - base);
        int j = 0;
        for (; j + U <= cnt; j += U) {
            V xv[U];
            f4 sd[U];
            int cj[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                cj[k] = __shfl(c, j + k, LPR);
                xv[k] = *(const V *)(a.src + (int64_t)cj[k] * a.ldsrc + foff);
                sd[k] = side_of<MODE>(a, cj[k], h);
            }
#pragma unroll
            for (int k = 0; k < U; ++k) add_entry<MODE, V>(a, o, row, cj[k], sd[k], xv[k], A1, A2, s);
        }
        for (; j < cnt; ++j) {
            const int c1 = __shfl(c, j, LPR);
            add_entry<MODE, V>(a, o, row, c1, side_of<MODE>(a, c1, h), *(const V *)(a.src + (int64_t)c1 * a.ldsrc + foff), A1, A2, s);
        }
    }
}

__device__ __forceinline__ float elu1(float y) { return y > 0.f ? y : expm1f(y); }

// the finished sums of VEC columns of a row, from column foff (head h), to their outputs
template <int VEC, int MODE>
__device__ __forceinline__ void finish(const GatArgs &a, int64_t row, int h, int64_t foff, typename vec_of<VEC>::type A1,
                                       typename vec_of<VEC>::type A2, float s)
{
    using V = typename vec_of<VEC>::type;
    if (MODE == FWD) {
        V y = V(0.f);
        if (s > 0.f) y = A1 / s;                                  // an empty row: exact zeros
        V o = y;
        if (a.epi == EPI_RELU || a.bias) {                        // PyG form: the bias, then ReLU and dropout
            float *po = (float *)&o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float t = a.bias ? po[k] + a.bias[foff + k] : po[k];
                if (a.epi == EPI_RELU) {
                    t = t > 0.f ? t : 0.f;
                    if (a.fdrop) t = ctgcn_u01(a.fkey, (uint64_t)row, (uint64_t)(foff + k)) >= a.p_feat ? t * a.fscale : 0.f;
                }
                po[k] = t;
            }
            *(V *)(a.out2 + row * a.ld2 + foff) = y;
        } else if (a.epi != EPI_NONE) {
            float *po = (float *)&o;
            const float *py = (const float *)&y;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float t = elu1(py[k]);
                if (a.fdrop) t = ctgcn_u01(a.fkey, (uint64_t)row, (uint64_t)(foff + k)) >= a.p_feat ? t * a.fscale : 0.f;
                po[k] = t;
            }
            *(V *)(a.out2 + row * a.ld2 + foff) = y;
        }
        *(V *)(a.out1 + row * a.ld1 + foff) = o;
    } else {
        if (a.out1) *(V *)(a.out1 + row * a.ld1 + foff) = A1;
        if (MODE == COL) *(V *)(a.out2 + row * a.ld2 + foff) = A2;
    }
    if (foff % a.F == 0) a.sout[row * a.heads + h] = s;
}

// every row that is not long
template <int VEC, int LPR, int MODE>
__global__ __launch_bounds__(256) void gat_row_kernel(const GatArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    const int start = a.row_ptr[row], end = a.row_ptr[row + 1];
    if (a.n_long > 0 && end - start > a.long_thresh) return;      // long row: gat_piece_kernel + gat_final_kernel
    for (int p0 = 0; p0 < a.chunks; p0 += LPR) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        // dead lanes work on chunk 0 (valid memory) and never store: keeps every load unconditional
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        const int h = (int)(foff / a.F);
        const Own o = own_of<MODE>(a, row, h);
        V A1 = V(0.f), A2 = V(0.f);
        float s = 0.f;
        if (MODE == ROW && a.ctr) A2 = *(const V *)(a.ctr + row * a.ldctr + foff);
        row_sum<VEC, LPR, MODE>(a, o, row, h, start, end, lig, foff, A1, A2, s);
        if (live) finish<VEC, MODE>(a, row, h, foff, A1, A2, s);
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of long row i into part[i][p]; its eight lane groups take interleaved entries
// and are added in group order
template <int VEC, int MODE>
__global__ __launch_bounds__(PIECE_THREADS) void gat_piece_kernel(const GatArgs a)
{
    using V = typename vec_of<VEC>::type;
    __shared__ V sm1[PIECE_GROUPS][PIECE_LANES];
    __shared__ V sm2[PIECE_GROUPS][PIECE_LANES];
    __shared__ float sms[PIECE_GROUPS][PIECE_LANES];
    const int64_t row = a.long_rows[blockIdx.y];
    const int start = a.row_ptr[row], len = a.row_ptr[row + 1] - start;
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const int p = blockIdx.x;
    if (p >= np) return;
    const int plen = (len + np - 1) / np;
    const int lo = start + min(len, p * plen), hi = start + min(len, (p + 1) * plen);
    const int lig = threadIdx.x & (PIECE_LANES - 1), g = threadIdx.x / PIECE_LANES;
    float *dst = a.part + ((int64_t)blockIdx.y * a.max_pieces + p) * a.piece_ld;

    for (int p0 = 0; p0 < a.chunks; p0 += PIECE_LANES) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        const int h = (int)(foff / a.F);
        const Own o = own_of<MODE>(a, row, h);
        V A1 = V(0.f), A2 = V(0.f);
        float s = 0.f;
        if (MODE == ROW && a.ctr) A2 = *(const V *)(a.ctr + row * a.ldctr + foff);
        for (int e = lo + g; e < hi; e += PIECE_GROUPS) {
            const int c = a.col[e];
            add_entry<MODE, V>(a, o, row, c, side_of<MODE>(a, c, h), *(const V *)(a.src + (int64_t)c * a.ldsrc + foff), A1, A2, s);
        }
        sm1[g][lig] = A1;
        sm2[g][lig] = A2;
        sms[g][lig] = s;
        __syncthreads();
        if (g == 0 && live) {
            V t1 = sm1[0][lig], t2 = sm2[0][lig];
            float ts = sms[0][lig];
#pragma unroll
            for (int k = 1; k < PIECE_GROUPS; ++k) {
                t1 += sm1[k][lig];
                t2 += sm2[k][lig];
                ts += sms[k][lig];
            }
            *(V *)(dst + foff) = t1;
            if (MODE == COL) *(V *)(dst + a.part_ld + foff) = t2;
            if (foff % a.F == 0) dst[2 * a.part_ld + h] = ts;
        }
        __syncthreads();
    }
}

// one wave per long row: the pieces in piece order, then the row's finish
template <int MODE>
__global__ __launch_bounds__(64) void gat_final_kernel(const GatArgs a)
{
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.piece_ld;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        const int h = c / a.F;
        float t1 = src[c], t2 = MODE == COL ? src[a.part_ld + c] : 0.f, ts = src[2 * a.part_ld + h];
        for (int p = 1; p < np; ++p) {
            const float *q = src + (int64_t)p * a.piece_ld;
            t1 += q[c];
            if (MODE == COL) t2 += q[a.part_ld + c];
            ts += q[2 * a.part_ld + h];
        }
        finish<1, MODE>(a, row, h, c, t1, t2, ts);
    }
}

// ------------------------------------------------------------------------------------------------ the row maximum m
// m[i][h] = -leakyrelu(u[i][h] + min_j v[col_j][h]) (0 for an empty row); MIN_LANES lanes per row, a block per long row.  With
// lsign = +1 the logit increases in v: the minimum is taken of -v and m = leakyrelu(u + max_j v).
__device__ __forceinline__ float shift_of(float u, float vmin, float alpha, float lsign)
{
    const float z = u - lsign * vmin;
    return lsign * (z > 0.f ? z : alpha * z);
}

__global__ __launch_bounds__(256) void gat_rowmax_kernel(int64_t n, int32_t heads, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                         const float *__restrict__ u, const float *__restrict__ v, float alpha, float lsign,
                                                         float *__restrict__ m, int32_t n_long, int32_t long_thresh)
{
    const int lig = threadIdx.x & (MIN_LANES - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / MIN_LANES) + threadIdx.x / MIN_LANES;
    if (row >= n) return;
    const int start = row_ptr[row], end = row_ptr[row + 1];
    if (n_long > 0 && end - start > long_thresh) return;
    for (int h = 0; h < heads; ++h) {
        float mn = INFINITY;
        for (int e = start + lig; e < end; e += MIN_LANES) mn = fminf(mn, -lsign * v[(int64_t)col[e] * heads + h]);
#pragma unroll
        for (int o = MIN_LANES / 2; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, MIN_LANES));
        if (lig == 0) m[row * heads + h] = end > start ? shift_of(u[row * heads + h], mn, alpha, lsign) : 0.f;
    }
}

__global__ __launch_bounds__(256) void gat_rowmax_long_kernel(int32_t heads, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                              const float *__restrict__ u, const float *__restrict__ v, float alpha, float lsign,
                                                              float *__restrict__ m, const int32_t *__restrict__ long_rows)
{
    __shared__ float sm[4];
    const int64_t row = long_rows[blockIdx.x];
    const int start = row_ptr[row], end = row_ptr[row + 1];
    for (int h = 0; h < heads; ++h) {
        float mn = INFINITY;
        for (int e = start + threadIdx.x; e < end; e += 256) mn = fminf(mn, -lsign * v[(int64_t)col[e] * heads + h]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mn;
        __syncthreads();
        if (threadIdx.x == 0) m[row * heads + h] = shift_of(u[row * heads + h], fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3])), alpha, lsign);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ passes over (row, head) pairs
// W lanes (a power of two up to 64, from F) own a pair and lie across the head's F columns; sums over them by xor shuffles
constexpr int SCORES = 0, PREP = 1, DU = 2, FINISH = 3;

struct PairArgs {
    int64_t pairs;
    int32_t heads, F, wshift;
    const float *X;         // SCORES, FINISH: S; PREP: dY; DU: G
    int64_t ldx;
    const float *Y;         // PREP: Y before the epilogue; DU: R; FINISH: B
    int64_t ldy;
    const float *a_src, *a_dst;   // [heads, F]: SCORES, FINISH
    float *o1, *o2;         // SCORES: u, v; DU: du; FINISH: dv
    const float *s1;        // PREP: u; DU: c; FINISH: k
    const float *s2;        // PREP: m; FINISH: du
    const float *s3;        // PREP: Z
    f4 *pack;               // PREP: written; DU: read
    float *G;               // PREP: G (null: G = dY); FINISH: dS, holding A (null: dv alone)
    int64_t ldg;
    int32_t epi, fdrop;
    double p_feat;
    float fscale;
    uint64_t fkey;
    float dsign;            // DU, FINISH: dz / dl's sign, +1 the reference's layer (dz = -s dl is in the formulas), -1 PyG's
};

template <int KIND>
__global__ __launch_bounds__(256) void gat_pair_kernel(const PairArgs a)
{
    const int W = 1 << a.wshift;
    const int l = threadIdx.x & (W - 1);
    const int64_t pair = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> a.wshift;
    if (pair >= a.pairs) return;
    const int64_t i = pair / a.heads;
    const int h = (int)(pair - i * a.heads);
    const int64_t c0 = (int64_t)h * a.F;
    const float *x = a.X + i * a.ldx + c0;
    float t1 = 0.f, t2 = 0.f;
    if (KIND == SCORES) {
        for (int c = l; c < a.F; c += W) {
            t1 = fmaf(x[c], a.a_src[c0 + c], t1);
            t2 = fmaf(x[c], a.a_dst[c0 + c], t2);
        }
    } else if (KIND == PREP) {
        const float *y = a.Y + i * a.ldy + c0;
        for (int c = l; c < a.F; c += W) {
            float g = x[c];
            if (a.epi != EPI_NONE) {
                if (!(y[c] > 0.f)) g *= expf(y[c]);               // ELU's derivative; at 0 it is 1 either way
                if (a.fdrop) g = ctgcn_u01(a.fkey, (uint64_t)i, (uint64_t)(c0 + c)) >= a.p_feat ? g * a.fscale : 0.f;
                a.G[i * a.ldg + c0 + c] = g;
            }
            t1 = fmaf(g, y[c], t1);
        }
    } else {
        const float *y = a.Y + i * a.ldy + c0;
        for (int c = l; c < a.F; c += W) t1 = fmaf(x[c], y[c], t1);
    }
    for (int o = W >> 1; o > 0; o >>= 1) {
        t1 += __shfl_xor(t1, o, 64);
        if (KIND == SCORES) t2 += __shfl_xor(t2, o, 64);
    }
    if (KIND == SCORES) {
        if (l == 0) { a.o1[pair] = t1; a.o2[pair] = t2; }
    } else if (KIND == PREP) {
        if (l == 0) { const float Z = a.s3[pair]; a.pack[pair] = f4{a.s1[pair], a.s2[pair], Z > 0.f ? 1.f / Z : 0.f, t1}; }
    } else if (KIND == DU) {
        if (l == 0) a.o1[pair] = a.dsign * fmaf(a.pack[pair].w, a.s1[pair], -t1);
    } else {
        const float dv = a.dsign * (a.s1[pair] - t1);
        if (l == 0) a.o1[pair] = dv;
        if (a.G) {
            const float du = a.s2[pair];
            float *ds = a.G + i * a.ldg + c0;
            for (int c = l; c < a.F; c += W) ds[c] = fmaf(dv, a.a_dst[c0 + c], fmaf(du, a.a_src[c0 + c], ds[c]));
        }
    }
}

// ------------------------------------------------------------------------------------------------ da_src, da_dst
// da[h][c] = sum_i dz[i][h] S[i][hF + c] for dz = du and dz = dv from one read of S: per-block column sums over DA_ROWS rows (wave w
// takes the block's rows w, w + 4, ..., the waves are added in wave order), then the blocks in block order by gat_da_sum_kernel
constexpr int DA_ROWS = 64, DA_WAVES = 4;
constexpr int DS_COLS = 32, DS_SEGS = 32;

// grid (row blocks, strips of 64 columns)
__global__ __launch_bounds__(64 * DA_WAVES) void gat_da_kernel(int64_t n, int32_t d, int32_t heads, int32_t F, const float *__restrict__ S, int64_t lds,
                                                               const float *__restrict__ du, const float *__restrict__ dv, int32_t part_ld,
                                                               float *__restrict__ part)
{
    __shared__ float sm[2][DA_WAVES][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * DA_ROWS;
    const int64_t row1 = min(n, row0 + DA_ROWS);
    const int c = blockIdx.y * 64 + lane;
    float t1 = 0.f, t2 = 0.f;
    if (c < d) {
        const int h = c / F;
#pragma unroll 4
        for (int64_t r = row0 + w; r < row1; r += DA_WAVES) {
            const float x = S[r * lds + c];
            if (du) t1 = fmaf(du[r * heads + h], x, t1);
            if (dv) t2 = fmaf(dv[r * heads + h], x, t2);
        }
    }
    sm[0][w][lane] = t1;
    sm[1][w][lane] = t2;
    __syncthreads();
    if (w == 0 && c < d) {
#pragma unroll
        for (int k = 1; k < DA_WAVES; ++k) {
            t1 += sm[0][k][lane];
            t2 += sm[1][k][lane];
        }
        float *dst = part + (int64_t)blockIdx.x * 2 * part_ld;
        dst[c] = t1;
        dst[part_ld + c] = t2;
    }
}

// out[c] = sum over the blocks of part[b][which][c]: DS_SEGS runs of consecutive blocks, each in block order, then the runs in run order
__global__ __launch_bounds__(DS_COLS * DS_SEGS) void gat_da_sum_kernel(int64_t blocks, int32_t d, int32_t part_ld, const float *__restrict__ part,
                                                                       float *da_src, float *da_dst)
{
    __shared__ float sm[DS_SEGS][DS_COLS];
    float *out = blockIdx.y ? da_dst : da_src;
    if (!out) return;                                             // block-uniform
    const int cx = threadIdx.x % DS_COLS, seg = threadIdx.x / DS_COLS;
    const int64_t c = (int64_t)blockIdx.x * DS_COLS + cx;
    const int64_t per = (blocks + DS_SEGS - 1) / DS_SEGS;
    const int64_t lo = min(blocks, seg * per), hi = min(blocks, lo + per);
    float t = 0.f;
    if (c < d)
        for (int64_t b = lo; b < hi; ++b) t += part[(b * 2 + blockIdx.y) * part_ld + c];
    sm[seg][cx] = t;
    __syncthreads();
    if (seg == 0 && c < d) {
        for (int k = 1; k < DS_SEGS; ++k) t += sm[k][cx];
        out[c] = t;
    }
}

template <int KIND>
int launch_pairs(PairArgs a, int64_t n, hipStream_t st)
{
    a.pairs = n * a.heads;
    a.wshift = 0;
    while ((1 << a.wshift) < a.F && a.wshift < 6) ++a.wshift;
    const int64_t blocks = ((a.pairs << a.wshift) + 255) / 256;
    if (blocks > INT32_MAX) return ctgcn_fail(CTGCN_E_UNSUPPORTED, "gat", "n * heads too large for one launch");
    hipLaunchKernelGGL(gat_pair_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

template <int VEC, int MODE>
int launch(GatArgs a, hipStream_t st)
{
    a.chunks = (a.d + VEC - 1) / VEC;
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((gat_row_kernel<VEC, decltype(lpr)::value, MODE>), grid, dim3(256), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL((gat_piece_kernel<VEC, MODE>), grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(gat_final_kernel<MODE>, grid, dim3(64), 0, st, a); });
}

template <int MODE>
int dispatch(const GatArgs &a, bool v4, void *stream)
{
    return v4 ? launch<4, MODE>(a, (hipStream_t)stream) : launch<1, MODE>(a, (hipStream_t)stream);
}

int32_t piece_floats(int32_t d, int32_t heads) { return 2 * ((d + 3) & ~3) + ((heads + 3) & ~3); }

// the checks every entry point shares; 1 when n == 0 (nothing to do), a negative code on an error
int check_shape(const char *what, int64_t n, int32_t d, int32_t heads)
{
    if (n < 0 || n > INT32_MAX || d < 1 || heads < 1 || d % heads) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31, d >= 1, heads >= 1 and d a multiple of heads");
    return n == 0 ? 1 : 0;
}

// the CSR, attention-dropout and long-row fields of a gather
int set_gather(GatArgs &a, const char *what, int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, double alpha,
               double p_att, uint64_t key, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
               size_t workspace_bytes)
{
    if (!row_ptr || !col) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    a.n = n; a.d = d; a.heads = heads; a.F = d / heads; a.row_ptr = row_ptr; a.col = col;
    a.alpha = (float)alpha; a.drop = p_att > 0.0; a.p_att = p_att; a.att_scale = 1.0f / (1.0f - (float)p_att); a.key = key;
    a.part_ld = (d + 3) & ~3;
    a.piece_ld = piece_floats(d, heads);
    return set_long_rows(a, what, long_rows, n_long, long_threshold, a.piece_ld, workspace, workspace_bytes,
                         "long rows need a 16-byte aligned workspace of at least n_long * ctgcn_gat_piece_floats(d, heads) * 4 bytes (one piece per row)");
}

bool bad_scalars(const char *what, double alpha, double p_att, double p_feat, int32_t epi, int &rc)
{
    rc = CTGCN_OK;
    if (!std::isfinite(alpha)) rc = ctgcn_fail(CTGCN_E_INVALID, what, "alpha not finite");
    else if (bad_p(p_att) || bad_p(p_feat)) rc = ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    else if (epi != EPI_NONE && epi != EPI_ELU && epi != EPI_ELU_DROP) rc = ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none), 1 (ELU) or 2 (ELU + feature dropout)");
    return rc != CTGCN_OK;
}

// The three gathers behind the reference-form entry points (lsign -1, no bias) and the PyG-form ones (lsign +1).  The PyG form has no
// attention dropout; its epi is 0 or 1 (ReLU, then dropout when p_feat > 0), and Y is written whenever out differs from it.
int fwd_impl(const char *what, float lsign, int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S,
             int64_t lds, const float *a_src, const float *a_dst, double alpha, const float *bias, int32_t epi, double p_att, uint64_t key,
             double p_feat, uint64_t fkey, float *out, int64_t ldout, float *Y, int64_t ldy, float *u, float *v, float *m, float *Z,
             const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool pyg = lsign > 0.f;
    int rc = check_shape(what, n, d, heads);
    if (rc < 0) return rc;
    if (pyg) {
        if (bad_scalars(what, alpha, 0.0, p_feat, EPI_NONE, rc)) return rc;
        if (epi != 0 && epi != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none) or 1 (ReLU, dropout)");
        epi = epi ? EPI_RELU : EPI_NONE;
    } else if (bad_scalars(what, alpha, p_att, p_feat, epi, rc)) return rc;
    const bool keep_y = epi != EPI_NONE || bias;
    if (lds < d || ldout < d || (keep_y && ldy < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n == 0) return CTGCN_OK;
    if (!S || !a_src || !a_dst || !out || !u || !v || !m || !Z || (keep_y && !Y)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    GatArgs a{};
    if ((rc = set_gather(a, what, n, d, heads, row_ptr, col, alpha, p_att, key, long_rows, n_long, long_threshold, workspace, workspace_bytes))) return rc;
    a.lsign = lsign; a.bias = bias;
    hipStream_t st = (hipStream_t)stream;
    PairArgs s{};
    s.heads = heads; s.F = a.F; s.X = S; s.ldx = lds; s.a_src = a_src; s.a_dst = a_dst; s.o1 = u; s.o2 = v;
    if ((rc = launch_pairs<SCORES>(s, n, st))) return rc;
    hipLaunchKernelGGL(gat_rowmax_kernel, dim3((unsigned)((n + 256 / MIN_LANES - 1) / (256 / MIN_LANES))), dim3(256), 0, st, n, heads, row_ptr, col,
                       (const float *)u, (const float *)v, a.alpha, lsign, m, n_long, long_threshold);
    CTGCN_TRY(hipGetLastError());
    if (n_long > 0) {
        hipLaunchKernelGGL(gat_rowmax_long_kernel, dim3((unsigned)n_long), dim3(256), 0, st, heads, row_ptr, col, (const float *)u, (const float *)v,
                           a.alpha, lsign, m, long_rows);
        CTGCN_TRY(hipGetLastError());
    }
    a.src = S; a.ldsrc = lds; a.u = u; a.v = v; a.m = m;
    a.out1 = out; a.ld1 = ldout; a.out2 = keep_y ? Y : nullptr; a.ld2 = ldy; a.sout = Z;
    a.epi = epi; a.fdrop = (epi == EPI_ELU_DROP || epi == EPI_RELU) && p_feat > 0.0; a.p_feat = p_feat; a.fscale = 1.0f / (1.0f - (float)p_feat); a.fkey = fkey;
    return dispatch<FWD>(a, float4_rows(a.F, {{S, lds}, {out, ldout}, {a.out2, ldy}}), stream);
}

}  // namespace

extern "C" int32_t ctgcn_gat_piece_floats(int32_t d, int32_t heads) { return (d < 1 || heads < 1) ? 0 : piece_floats(d, heads); }

extern "C" int ctgcn_gat_fwd_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                                 const float *a_src, const float *a_dst, double alpha, int32_t epi, double p_att, uint64_t key, double p_feat,
                                 uint64_t fkey, float *out, int64_t ldout, float *Y, int64_t ldy, float *u, float *v, float *m, float *Z,
                                 const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                                 void *stream)
{
    return fwd_impl("gat_fwd", -1.f, n, d, heads, row_ptr, col, S, lds, a_src, a_dst, alpha, nullptr, epi, p_att, key, p_feat, fkey, out, ldout, Y, ldy,
                    u, v, m, Z, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_tgat_fwd_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                                  const float *a_tgt, const float *a_src, double slope, const float *bias, int32_t epi, double p, uint64_t key,
                                  float *out, int64_t ldout, float *Y, int64_t ldy, float *u, float *v, float *m, float *Z,
                                  const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    return fwd_impl("tgat_fwd", 1.f, n, d, heads, row_ptr, col, S, lds, a_tgt, a_src, slope, bias, epi, 0.0, 0, p, key, out, ldout, Y, ldy, u, v, m, Z,
                    long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_gat_bwd_prep_f32(int64_t n, int32_t d, int32_t heads, const float *dY, int64_t lddy, const float *Y, int64_t ldy, int32_t epi,
                                      double p_feat, uint64_t fkey, const float *u, const float *m, const float *Z, float *G, int64_t ldg,
                                      void *pack, void *stream)
{
    const char *what = "gat_bwd_prep";
    int rc = check_shape(what, n, d, heads);
    if (rc < 0) return rc;
    if (bad_scalars(what, 0.0, 0.0, p_feat, epi, rc)) return rc;
    if (lddy < d || ldy < d || (epi != EPI_NONE && ldg < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n == 0) return CTGCN_OK;
    if (!dY || !Y || !u || !m || !Z || !pack || (epi != EPI_NONE && !G)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!ctgcn_aligned16(pack)) return ctgcn_fail(CTGCN_E_INVALID, what, "pack must be 16-byte aligned");
    PairArgs s{};
    s.heads = heads; s.F = d / heads; s.X = dY; s.ldx = lddy; s.Y = Y; s.ldy = ldy; s.s1 = u; s.s2 = m; s.s3 = Z; s.pack = (f4 *)pack;
    s.G = epi != EPI_NONE ? G : nullptr; s.ldg = ldg; s.epi = epi; s.fdrop = epi == EPI_ELU_DROP && p_feat > 0.0; s.p_feat = p_feat;
    s.fscale = 1.0f / (1.0f - (float)p_feat); s.fkey = fkey;
    return launch_pairs<PREP>(s, n, (hipStream_t)stream);
}

namespace {

int bwd_row_impl(const char *what, float lsign, int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S,
                 int64_t lds, const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *v, const void *pack, double alpha,
                 double p_att, uint64_t key, float *R, int64_t ldr, float *csum, float *du, const int32_t *long_rows, int32_t n_long,
                 int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    const bool pyg = lsign > 0.f;                                 // Y: the PyG form's centre of the gathered rows; null in the reference form
    int rc = check_shape(what, n, d, heads);
    if (rc < 0) return rc;
    if (bad_scalars(what, alpha, p_att, 0.0, EPI_NONE, rc)) return rc;
    if (lds < d || ldg < d || ldr < d || (pyg && ldy < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n == 0) return CTGCN_OK;
    if (!S || !G || !v || !pack || !R || !csum || !du || (pyg && !Y)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!ctgcn_aligned16(pack)) return ctgcn_fail(CTGCN_E_INVALID, what, "pack must be 16-byte aligned");
    GatArgs a{};
    if ((rc = set_gather(a, what, n, d, heads, row_ptr, col, alpha, p_att, key, long_rows, n_long, long_threshold, workspace, workspace_bytes))) return rc;
    a.src = S; a.ldsrc = lds; a.v = v; a.pack = (const f4 *)pack; a.out1 = R; a.ld1 = ldr; a.sout = csum; a.lsign = lsign;
    a.ctr = pyg ? Y : nullptr; a.ldctr = ldy;
    if ((rc = dispatch<ROW>(a, float4_rows(a.F, {{S, lds}, {R, ldr}, {a.ctr, ldy}}), stream))) return rc;
    PairArgs s{};
    s.heads = heads; s.F = a.F; s.X = G; s.ldx = ldg; s.Y = R; s.ldy = ldr; s.s1 = csum; s.pack = (f4 *)pack; s.o1 = du; s.dsign = -lsign;
    return launch_pairs<DU>(s, n, (hipStream_t)stream);
}

int bwd_col_impl(const char *what, float lsign, int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *G,
                 int64_t ldg, const float *S, int64_t lds, const float *v, const void *pack, const float *a_src, const float *a_dst, double alpha,
                 double p_att, uint64_t key, const float *du, float *dS, int64_t ldds, float *B, int64_t ldb, float *ksum, float *dv,
                 const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_shape(what, n, d, heads);
    if (rc < 0) return rc;
    if (bad_scalars(what, alpha, p_att, 0.0, EPI_NONE, rc)) return rc;
    if (lds < d || ldg < d || ldb < d || (dS && ldds < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if ((dS == nullptr) != (du == nullptr)) return ctgcn_fail(CTGCN_E_INVALID, what, "du and dS go together");
    if (n == 0) return CTGCN_OK;
    if (!S || !G || !v || !pack || !B || !ksum || !dv || (dS && (!a_src || !a_dst))) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!ctgcn_aligned16(pack)) return ctgcn_fail(CTGCN_E_INVALID, what, "pack must be 16-byte aligned");
    GatArgs a{};
    if ((rc = set_gather(a, what, n, d, heads, row_ptr, col, alpha, p_att, key, long_rows, n_long, long_threshold, workspace, workspace_bytes))) return rc;
    a.src = G; a.ldsrc = ldg; a.v = v; a.pack = (const f4 *)pack; a.out1 = dS; a.ld1 = ldds; a.out2 = B; a.ld2 = ldb; a.sout = ksum; a.lsign = lsign;
    if ((rc = dispatch<COL>(a, float4_rows(a.F, {{G, ldg}, {dS, ldds}, {B, ldb}}), stream))) return rc;
    PairArgs s{};
    s.heads = heads; s.F = a.F; s.X = S; s.ldx = lds; s.Y = B; s.ldy = ldb; s.a_src = a_src; s.a_dst = a_dst; s.s1 = ksum; s.s2 = du; s.o1 = dv;
    s.G = dS; s.ldg = ldds; s.dsign = -lsign;
    return launch_pairs<FINISH>(s, n, (hipStream_t)stream);
}

}  // namespace

extern "C" int ctgcn_gat_bwd_row_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                                     const float *G, int64_t ldg, const float *v, const void *pack, double alpha, double p_att, uint64_t key,
                                     float *R, int64_t ldr, float *csum, float *du, const int32_t *long_rows, int32_t n_long,
                                     int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    return bwd_row_impl("gat_bwd_row", -1.f, n, d, heads, row_ptr, col, S, lds, G, ldg, nullptr, 0, v, pack, alpha, p_att, key, R, ldr, csum, du, long_rows, n_long,
                        long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_tgat_bwd_row_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                                      const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *v, const void *pack, double slope,
                                      float *R, int64_t ldr, float *csum, float *du, const int32_t *long_rows, int32_t n_long,
                                      int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    return bwd_row_impl("tgat_bwd_row", 1.f, n, d, heads, row_ptr, col, S, lds, G, ldg, Y, ldy, v, pack, slope, 0.0, 0, R, ldr, csum, du, long_rows, n_long,
                        long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_gat_bwd_col_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *G, int64_t ldg,
                                     const float *S, int64_t lds, const float *v, const void *pack, const float *a_src, const float *a_dst,
                                     double alpha, double p_att, uint64_t key, const float *du, float *dS, int64_t ldds, float *B, int64_t ldb,
                                     float *ksum, float *dv, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    return bwd_col_impl("gat_bwd_col", -1.f, n, d, heads, row_ptr, col, G, ldg, S, lds, v, pack, a_src, a_dst, alpha, p_att, key, du, dS, ldds, B, ldb,
                        ksum, dv, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_tgat_bwd_col_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *G, int64_t ldg,
                                      const float *S, int64_t lds, const float *v, const void *pack, const float *a_tgt, const float *a_src,
                                      double slope, const float *du, float *dS, int64_t ldds, float *B, int64_t ldb, float *ksum, float *dv,
                                      const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    return bwd_col_impl("tgat_bwd_col", 1.f, n, d, heads, row_ptr, col, G, ldg, S, lds, v, pack, a_tgt, a_src, slope, 0.0, 0, du, dS, ldds, B, ldb, ksum,
                        dv, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" size_t ctgcn_gat_da_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 0 || d < 1) return 0;
    return (size_t)((n + DA_ROWS - 1) / DA_ROWS) * 2 * (size_t)((d + 3) & ~3) * sizeof(float);
}

extern "C" int ctgcn_gat_da_f32(int64_t n, int32_t d, int32_t heads, const float *S, int64_t lds, const float *du, const float *dv, float *da_src,
                                float *da_dst, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "gat_da";
    int rc = check_shape(what, n, d, heads);
    if (rc < 0) return rc;
    if (lds < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if ((du == nullptr) != (da_src == nullptr) || (dv == nullptr) != (da_dst == nullptr)) return ctgcn_fail(CTGCN_E_INVALID, what, "du goes with da_src, dv with da_dst");
    if (!du && !dv) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                                                 // empty sums
        if (da_src) CTGCN_TRY(hipMemsetAsync(da_src, 0, (size_t)d * sizeof(float), st));
        if (da_dst) CTGCN_TRY(hipMemsetAsync(da_dst, 0, (size_t)d * sizeof(float), st));
        return CTGCN_OK;
    }
    if (!S) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!workspace || workspace_bytes < ctgcn_gat_da_workspace_bytes(n, d))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must hold ctgcn_gat_da_workspace_bytes() bytes");
    const int64_t blocks = (n + DA_ROWS - 1) / DA_ROWS;
    const int32_t part_ld = (d + 3) & ~3;
    hipLaunchKernelGGL(gat_da_kernel, dim3((unsigned)blocks, (unsigned)((d + 63) / 64)), dim3(64 * DA_WAVES), 0, st, n, d, heads, d / heads, S, lds, du, dv, part_ld, (float *)workspace);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(gat_da_sum_kernel, dim3((unsigned)((d + DS_COLS - 1) / DS_COLS), 2), dim3(DS_COLS * DS_SEGS), 0, st, blocks, d, part_ld,
                       (const float *)workspace, da_src, da_dst);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
