// ctgcn_gcn.hip — the GCN step of the EvolveGCN baseline (reference baseline/egcn.py:74, helper.py:27-47) on the GPU.
//
//   normalise   val_out = D^-1/2 A D^-1/2 (or D^-1 A) over a CSR that already holds the diagonal: row sums and the scale r_i in fp64, the
//               product r_i a_ij r_j in fp64, rounded to fp32 once — the reference's float64 scipy arithmetic followed by .float().
//   forward     Y[i] = act(sum_e val[e] S[col[e]]), optionally scores[i] = Y[i] · p for the next layer's top-k.
//   backward    dS[i] = sum_e val[e] (dY[col[e]] ∘ m(Y[col[e]])) over the same (symmetric) CSR; the mask is formed on the gathered row.
//
// Pull form (the scaffold and its contract: ctgcn_gather.h): a group of LPR lanes owns a destination row and a float4 (or a float) per
// lane of it, the row's entries are read LPR at a time and handed round by shuffles, four gathered rows in flight per group.  Rows
// longer than long_threshold entries are left to a block-per-piece kernel: a piece is at most 4 long_threshold entries, its eight lane
// groups sum interleaved entries and are added in group order, the pieces of a row are added in piece order by a last kernel that also
// finishes the row.  No atomics: every sum has a fixed order, so repeated launches are bit-identical.
//
// The GCN step of the GCN / GCRN baselines (reference baseline/gcn.py:36-43 and :84-88, baseline/gcrn.py:56-57) is the same gather with
// an epilogue on the finished row:
//   conv fwd    Y[i] = epi(sum_e val[e] S[col[e]] + b); epi none, ReLU with counter-based dropout (ctgcn_rng.h), or the row's L2
//               normalisation with the norm kept for the backward.
//   conv prep   the backward's one N x d pass: G = d loss / d (pre-epilogue sum) from dY and Y, and the bias gradient as per-block
//               column sums added in block order.  dS = Â^T G is then the conv forward without epilogue over the transposed CSR, so
//               the matrix need not be symmetric and no gather reads two rows per entry.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr float RRELU_SLOPE = (float)((1.0 / 8.0 + 1.0 / 3.0) / 2.0);   // F.rrelu in eval mode: the mean of its default bounds
constexpr int U = 4;                   // gathered rows in flight per lane group

__device__ __forceinline__ float rrelu1(float y) { return y >= 0.f ? y : y * RRELU_SLOPE; }
__device__ __forceinline__ f4 rrelu(f4 y) { return f4{rrelu1(y.x), rrelu1(y.y), rrelu1(y.z), rrelu1(y.w)}; }
__device__ __forceinline__ float rrelu(float y) { return rrelu1(y); }
// torch's leaky_relu backward: a pre-activation of exactly 0 takes the slope; sign(Y) = sign(pre-activation) as the slope is positive
__device__ __forceinline__ float mask1(float g, float y) { return y > 0.f ? g : g * RRELU_SLOPE; }
__device__ __forceinline__ f4 masked(f4 g, f4 y) { return f4{mask1(g.x, y.x), mask1(g.y, y.y), mask1(g.z, y.z), mask1(g.w, y.w)}; }
__device__ __forceinline__ float masked(float g, float y) { return mask1(g, y); }
__device__ __forceinline__ float vdot(f4 a, f4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float vdot(float a, float b) { return a * b; }

struct GcnArgs {
    int64_t n;
    int32_t d;
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    const float *src;       // forward: S; backward: dY
    int64_t ldsrc;
    const float *ymask;     // backward with act 1: Y (row stride ldmask); else null
    int64_t ldmask;
    float *out;             // forward: Y; backward: dS
    int64_t ldout;
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t chunks;         // ceil(d / VEC)
    int32_t max_pieces;     // pieces a long row may be cut into (what the workspace holds)
    int32_t part_ld;        // floats per partial vector: d rounded up to 4
    float *part;            // [n_long][max_pieces][part_ld]
};

template <int VEC, bool BWD>
__device__ __forceinline__ typename vec_of<VEC>::type gather_row(const GcnArgs &a, int64_t c, int64_t foff)
{
    using V = typename vec_of<VEC>::type;
    V x = *(const V *)(a.src + c * a.ldsrc + foff);
    if (BWD && a.ymask) x = masked(x, *(const V *)(a.ymask + c * a.ldmask + foff));
    return x;
}

// sum_e val[e] src[col[e]][foff ..] over the entries [start, end) of a row, by the row's LPR lanes: the entries are read LPR at a time
// and handed round by shuffles, U gathered rows in flight
template <int VEC, int LPR, bool BWD>
__device__ __forceinline__ typename vec_of<VEC>::type row_sum(const GcnArgs &a, int start, int end, int lig, int64_t foff)
{
    using V = typename vec_of<VEC>::type;
    V P = V(0.f);
    for (int base = start; base < end; base += LPR) {
        const int my = base + lig;
        int c = 0;
        float w = 0.f;
        if (my < end) {
            c = a.col[my];
            w = a.val[my];
        }
        const int cnt = min(LPR, end - base);
        int j = 0;
        for (; j + U <= cnt; j += U) {
            V xv[U];
            float wj[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cj = __shfl(c, j + u, LPR);
                wj[u] = __shfl(w, j + u, LPR);
                xv[u] = gather_row<VEC, BWD>(a, cj, foff);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) P = vfma(wj[u], xv[u], P);
        }
        for (; j < cnt; ++j) {
            const int cj = __shfl(c, j, LPR);
            const float w1 = __shfl(w, j, LPR);
            P = vfma(w1, gather_row<VEC, BWD>(a, cj, foff), P);
        }
    }
    return P;
}

// ------------------------------------------------------------------------------------------------ epilogues on a finished row
// 0..2 are ctgcn_gcn_conv_fwd_f32's epi argument; EPI_RRELU is the layer's act 1 and is not accepted there
constexpr int EPI_NONE = 0, EPI_RELU = 1, EPI_L2NORM = 2, EPI_RRELU = 3;

struct GcnEpi {
    int32_t kind;
    int32_t drop;           // RELU: p > 0
    const float *bias;      // [d] or null: added before the kind is applied
    const float *score_vec; // [d] or null: score_out[i] = Y[i] · score_vec
    float *score_out;
    float *norm;            // L2NORM: [n], the norm before the clamp
    double p;
    float scale;            // 1 / (1 - p)
    uint64_t key;
};

// relu, then dropout: entry (row, c) is kept iff ctgcn_u01(key, row, c) >= p
__device__ __forceinline__ float relu_drop(float v, const GcnEpi &e, int64_t row, int64_t c)
{
    if (!(v > 0.f)) return 0.f;
    if (!e.drop) return v;
    return ctgcn_u01(e.key, (uint64_t)row, (uint64_t)c) >= e.p ? v * e.scale : 0.f;
}
__device__ __forceinline__ f4 relu_drop(f4 v, const GcnEpi &e, int64_t row, int64_t c)
{
    return f4{relu_drop(v.x, e, row, c), relu_drop(v.y, e, row, c + 1), relu_drop(v.z, e, row, c + 2), relu_drop(v.w, e, row, c + 3)};
}
__device__ __forceinline__ float relu_grad(float g, float y, float scale) { return y > 0.f ? g * scale : 0.f; }
__device__ __forceinline__ f4 relu_grad(f4 g, f4 y, float scale)
{
    return f4{relu_grad(g.x, y.x, scale), relu_grad(g.y, y.y, scale), relu_grad(g.z, y.z, scale), relu_grad(g.w, y.w, scale)};
}

// every row that is not long.  KIND is e.kind: a template parameter, so that a path carries no registers for the epilogues it does
// not run.  The backward is the masked gather alone, KIND none: its instantiation compiles bias and score out too.
template <int VEC, int LPR, bool BWD, int KIND>
__global__ __launch_bounds__(256) void gcn_row_kernel(const GcnArgs a, const GcnEpi e)
{
    using V = typename vec_of<VEC>::type;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    const int start = a.row_ptr[row], end = a.row_ptr[row + 1];
    if (a.n_long > 0 && end - start > a.long_thresh) return;      // long row: gcn_piece_kernel + gcn_final_kernel
    const bool score = !BWD && e.score_vec;
    constexpr bool l2 = KIND == EPI_L2NORM;
    const bool one_pass = a.chunks <= LPR;                        // L2NORM: the row stays in registers until its norm is known
    float sc = 0.f, ss = 0.f;
    V P = V(0.f);

    for (int p0 = 0; p0 < a.chunks; p0 += LPR) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        // dead lanes read chunk 0 (valid memory) and never store: keeps every load unconditional
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        P = row_sum<VEC, LPR, BWD>(a, start, end, lig, foff);
        if (!BWD && e.bias) P += *(const V *)(e.bias + foff);
        if (KIND == EPI_RRELU) P = rrelu(P);
        else if (KIND == EPI_RELU) P = relu_drop(P, e, row, foff);
        if (live) {
            if (l2) ss += vdot(P, P);
            if (!(l2 && one_pass)) *(V *)(a.out + row * a.ldout + foff) = P;
            if (score) sc += vdot(P, *(const V *)(e.score_vec + foff));
        }
    }
    if (score) {
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) sc += __shfl_xor(sc, o, LPR);
        if (lig == 0) e.score_out[row] = sc;
    }
    if (!l2) return;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, LPR);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, L2_EPS);
    if (lig == 0) e.norm[row] = nrm;
    if (one_pass) {
        if (lig < a.chunks) *(V *)(a.out + row * a.ldout + (int64_t)lig * VEC) = P / den;
    } else {
        for (int ch = lig; ch < a.chunks; ch += LPR) {            // the chunks this lane wrote itself
            V *q = (V *)(a.out + row * a.ldout + (int64_t)ch * VEC);
            *q = *q / den;
        }
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of long row i into part[i][p]
template <int VEC, bool BWD>
__global__ __launch_bounds__(PIECE_THREADS) void gcn_piece_kernel(const GcnArgs a)
{
    using V = typename vec_of<VEC>::type;
    __shared__ V sm[PIECE_GROUPS][PIECE_LANES];
    const int64_t row = a.long_rows[blockIdx.y];
    const int start = a.row_ptr[row], len = a.row_ptr[row + 1] - start;
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const int p = blockIdx.x;
    if (p >= np) return;
    const int plen = (len + np - 1) / np;
    const int lo = start + min(len, p * plen), hi = start + min(len, (p + 1) * plen);
    const int lig = threadIdx.x & (PIECE_LANES - 1), g = threadIdx.x / PIECE_LANES;
    float *dst = a.part + ((int64_t)blockIdx.y * a.max_pieces + p) * a.part_ld;

    for (int p0 = 0; p0 < a.chunks; p0 += PIECE_LANES) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
        for (int e = lo + g; e < hi; e += PIECE_GROUPS) P = vfma(a.val[e], gather_row<VEC, BWD>(a, a.col[e], foff), P);
        sm[g][lig] = P;
        __syncthreads();
        if (g == 0 && live) {
            V t = sm[0][lig];
#pragma unroll
            for (int k = 1; k < PIECE_GROUPS; ++k) t += sm[k][lig];
            *(V *)(dst + foff) = t;
        }
        __syncthreads();
    }
}

// one wave per long row: the pieces in piece order, the bias, the epilogue, the row and its score
__global__ __launch_bounds__(64) void gcn_final_kernel(const GcnArgs a, const GcnEpi e)
{
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    float sc = 0.f, ss = 0.f;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        float t = src[c];
        for (int p = 1; p < np; ++p) t += src[(int64_t)p * a.part_ld + c];
        if (e.bias) t += e.bias[c];
        if (e.kind == EPI_RRELU) t = rrelu1(t);
        else if (e.kind == EPI_RELU) t = relu_drop(t, e, row, c);
        ss = fmaf(t, t, ss);
        a.out[row * a.ldout + c] = t;
        if (e.score_vec) sc = fmaf(t, e.score_vec[c], sc);
    }
    if (e.score_vec) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
        if (threadIdx.x == 0) e.score_out[row] = sc;
    }
    if (e.kind != EPI_L2NORM) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, L2_EPS);
    if (threadIdx.x == 0) e.norm[row] = nrm;
    for (int c = threadIdx.x; c < a.d; c += 64) a.out[row * a.ldout + c] /= den;
}

// ------------------------------------------------------------------------------------------------ GCN / GCRN step: backward pre-pass
// PREP_ROWS rows a block, one partial bias-gradient vector per block; colsum_kernel (ctgcn_gather.h) adds them in block order
struct PrepArgs {
    int64_t n;
    int32_t d, chunks, epi;
    const float *dY;
    int64_t lddy;
    const float *Y;
    int64_t ldy;
    const float *norm;
    float scale;
    float *G;               // null: only the column sums are wanted (EPI_NONE)
    int64_t ldg;
    float *part;            // [blocks][part_ld] or null
    int32_t part_ld;
};

template <int VEC>
__global__ __launch_bounds__(64 * PREP_WAVES) void gcn_conv_prep_kernel(const PrepArgs a)
{
    using V = typename vec_of<VEC>::type;
    __shared__ V sm[PREP_WAVES][64];
    __shared__ float s_dot[PREP_ROWS], s_den[PREP_ROWS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;

    if (a.epi == EPI_L2NORM) {
        for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
            const int64_t r = row0 + k;
            float dot = 0.f;
            for (int ch = lane; ch < a.chunks; ch += 64)
                dot += vdot(*(const V *)(a.Y + r * a.ldy + (int64_t)ch * VEC), *(const V *)(a.dY + r * a.lddy + (int64_t)ch * VEC));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
            if (lane == 0) {
                const float nrm = a.norm[r];
                const bool ok = nrm >= L2_EPS;                    // below the clamp the denominator was the constant eps
                s_dot[k] = ok ? dot : 0.f;
                s_den[k] = ok ? nrm : L2_EPS;
            }
        }
        __syncthreads();
    }
    for (int p0 = 0; p0 < a.chunks; p0 += 64) {
        const int ch = p0 + lane;
        const bool live = ch < a.chunks;
        const int64_t foff = (int64_t)ch * VEC;
        V acc = V(0.f);
        if (live) {
            for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
                const int64_t r = row0 + k;
                V g = *(const V *)(a.dY + r * a.lddy + foff);
                if (a.epi == EPI_RELU) g = relu_grad(g, *(const V *)(a.Y + r * a.ldy + foff), a.scale);
                else if (a.epi == EPI_L2NORM) g = (g - *(const V *)(a.Y + r * a.ldy + foff) * s_dot[k]) / s_den[k];
                if (a.G) *(V *)(a.G + r * a.ldg + foff) = g;
                acc += g;
            }
        }
        if (a.part) {                                             // block-uniform
            sm[w][lane] = acc;
            __syncthreads();
            if (w == 0 && live) {
                V t = sm[0][lane];
#pragma unroll
                for (int k = 1; k < PREP_WAVES; ++k) t += sm[k][lane];
                *(V *)(a.part + (int64_t)blockIdx.x * a.part_ld + foff) = t;
            }
            __syncthreads();
        }
    }
}

template <int VEC, bool BWD, int KIND>
int launch(GcnArgs a, const GcnEpi &e, hipStream_t st)
{
    a.chunks = (a.d + VEC - 1) / VEC;
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((gcn_row_kernel<VEC, decltype(lpr)::value, BWD, KIND>), grid, dim3(256), 0, st, a, e); },
        [&](dim3 grid) { hipLaunchKernelGGL((gcn_piece_kernel<VEC, BWD>), grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(gcn_final_kernel, grid, dim3(64), 0, st, a, e); });
}

// picks the launcher's instantiation for a call: float4 or scalar rows, the backward's masked gather or the forward with e.kind
int dispatch(const GcnArgs &a, const GcnEpi &e, bool bwd, bool v4, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (bwd) return v4 ? launch<4, true, EPI_NONE>(a, e, st) : launch<1, true, EPI_NONE>(a, e, st);
    switch (e.kind) {
    case EPI_RELU: return v4 ? launch<4, false, EPI_RELU>(a, e, st) : launch<1, false, EPI_RELU>(a, e, st);
    case EPI_L2NORM: return v4 ? launch<4, false, EPI_L2NORM>(a, e, st) : launch<1, false, EPI_L2NORM>(a, e, st);
    case EPI_RRELU: return v4 ? launch<4, false, EPI_RRELU>(a, e, st) : launch<1, false, EPI_RRELU>(a, e, st);
    default: return v4 ? launch<4, false, EPI_NONE>(a, e, st) : launch<1, false, EPI_NONE>(a, e, st);
    }
}

// checks shared by the three gather entry points; fills the long-row fields
int set_common(GcnArgs &a, const char *what, int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val,
               const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes)
{
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.n = n; a.d = d; a.row_ptr = row_ptr; a.col = col; a.val = val;
    a.part_ld = (d + 3) & ~3;
    return set_long_rows(a, what, long_rows, n_long, long_threshold, a.part_ld, workspace, workspace_bytes,
                         "long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (one piece per row)");
}

bool bad_epi(int32_t epi) { return epi != EPI_NONE && epi != EPI_RELU && epi != EPI_L2NORM; }

// ------------------------------------------------------------------------------------------------ normalisation
constexpr int NORM_LANES = 16;

__global__ __launch_bounds__(256) void gcn_rowscale_kernel(int64_t n, const int32_t *__restrict__ row_ptr, const float *__restrict__ val,
                                                           int row_norm, double *__restrict__ r, int32_t *flag)
{
    const int lig = threadIdx.x & (NORM_LANES - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;
    if (row >= n) return;
    double s = 0.0;
    for (int e = row_ptr[row] + lig, end = row_ptr[row + 1]; e < end; e += NORM_LANES) s += (double)val[e];
#pragma unroll
    for (int o = NORM_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, NORM_LANES);
    if (lig) return;
    if (s < 0.0) *flag = 1;                       // every writer stores the same value
    r[row] = s == 0.0 ? 0.0 : (row_norm ? 1.0 / s : 1.0 / sqrt(s));
}

__global__ __launch_bounds__(256) void gcn_scale_kernel(int64_t n, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ val, int row_norm, const double *__restrict__ r,
                                                        float *__restrict__ out)
{
    const int lig = threadIdx.x & (NORM_LANES - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;
    if (row >= n) return;
    const double ri = r[row];
    for (int e = row_ptr[row] + lig, end = row_ptr[row + 1]; e < end; e += NORM_LANES) {
        const double v = ri * (double)val[e];
        out[e] = (float)(row_norm ? v : v * r[col[e]]);
    }
}

}  // namespace

extern "C" size_t ctgcn_gcn_normalize_workspace_bytes(int64_t n) { return n < 0 ? 0 : (size_t)n * sizeof(double); }

extern "C" int ctgcn_gcn_normalize_f32(int64_t n, const int32_t *row_ptr, const int32_t *col, const float *val_in, int32_t row_norm,
                                       float *val_out, int32_t *flag, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_normalize";
    if (n < 0 || n > INT32_MAX) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31");
    if (row_norm != 0 && row_norm != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "row_norm must be 0 or 1");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val_in || !val_out || !flag) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < ctgcn_gcn_normalize_workspace_bytes(n))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 8-byte aligned and hold ctgcn_gcn_normalize_workspace_bytes() bytes");
    hipStream_t st = (hipStream_t)stream;
    double *r = (double *)workspace;
    const unsigned grid = (unsigned)((n + 256 / NORM_LANES - 1) / (256 / NORM_LANES));
    CTGCN_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(gcn_rowscale_kernel, dim3(grid), dim3(256), 0, st, n, row_ptr, val_in, (int)row_norm, r, flag);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(gcn_scale_kernel, dim3(grid), dim3(256), 0, st, n, row_ptr, col, val_in, (int)row_norm, (const double *)r, val_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_gcn_layer_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                       int64_t lds, float *Y, int64_t ldy, int32_t act, const float *score_vec, float *score_out,
                                       const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_layer_fwd";
    GcnArgs a{};
    if (act != 0 && act != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (eval-mode RReLU)");
    if (lds < d || ldy < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if ((score_vec == nullptr) != (score_out == nullptr)) return ctgcn_fail(CTGCN_E_INVALID, what, "score_vec and score_out go together");
    if (int rc = set_common(a, what, n, d, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!S || !Y) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = S; a.ldsrc = lds; a.out = Y; a.ldout = ldy;
    GcnEpi e{};
    e.kind = act ? EPI_RRELU : EPI_NONE; e.score_vec = score_vec; e.score_out = score_out;
    return dispatch(a, e, false, float4_rows(d, {{S, lds}, {Y, ldy}, {score_vec, 0}}), stream);
}

extern "C" int ctgcn_gcn_layer_bwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *dY,
                                       int64_t lddy, const float *Y, int64_t ldy, int32_t act, float *dS, int64_t ldds,
                                       const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_layer_bwd";
    GcnArgs a{};
    if (act != 0 && act != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (eval-mode RReLU)");
    if (lddy < d || ldds < d || (act && ldy < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (int rc = set_common(a, what, n, d, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!dY || !dS || (act && !Y)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = dY; a.ldsrc = lddy; a.ymask = act ? Y : nullptr; a.ldmask = act ? ldy : 0; a.out = dS; a.ldout = ldds;
    return dispatch(a, GcnEpi{}, true, float4_rows(d, {{dY, lddy}, {dS, ldds}, {a.ymask, ldy}}), stream);
}

extern "C" int ctgcn_gcn_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                      int64_t lds, const float *bias, float *Y, int64_t ldy, int32_t epi, double p, uint64_t key,
                                      float *norm, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_conv_fwd";
    GcnArgs a{};
    if (bad_epi(epi)) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none), 1 (ReLU + dropout) or 2 (L2 row normalisation)");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (lds < d || ldy < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (int rc = set_common(a, what, n, d, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!S || !Y || (epi == EPI_L2NORM && !norm)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = S; a.ldsrc = lds; a.out = Y; a.ldout = ldy;
    GcnEpi e{};
    e.kind = epi; e.bias = bias; e.norm = norm; e.drop = epi == EPI_RELU && p > 0.0; e.p = p; e.scale = 1.0f / (1.0f - (float)p); e.key = key;
    return dispatch(a, e, false, float4_rows(d, {{S, lds}, {Y, ldy}, {bias, 0}}), stream);
}

extern "C" int32_t ctgcn_gcn_conv_prep_rows(void) { return PREP_ROWS; }

extern "C" size_t ctgcn_gcn_conv_prep_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 0 || d < 1) return 0;
    return (size_t)((n + PREP_ROWS - 1) / PREP_ROWS) * (size_t)((d + 3) & ~3) * sizeof(float);
}

extern "C" int ctgcn_gcn_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *norm,
                                       int32_t epi, double p, float *G, int64_t ldg, float *db, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    const char *what = "gcn_conv_prep";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (bad_epi(epi)) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none), 1 (ReLU + dropout) or 2 (L2 row normalisation)");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (n == 0) return CTGCN_OK;
    const bool wants_g = epi != EPI_NONE;
    if (!dY || (wants_g && (!Y || !G)) || (epi == EPI_L2NORM && !norm)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (lddy < d || (wants_g && (ldy < d || ldg < d))) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (db && (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < ctgcn_gcn_conv_prep_workspace_bytes(n, d)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "a bias gradient needs a 16-byte aligned workspace of ctgcn_gcn_conv_prep_workspace_bytes() bytes");
    if (!wants_g && !db) return CTGCN_OK;                          // G = dY and no column sums: nothing to write
    PrepArgs a{};
    a.n = n; a.d = d; a.epi = epi; a.dY = dY; a.lddy = lddy; a.Y = wants_g ? Y : nullptr; a.ldy = ldy; a.norm = norm;
    a.scale = epi == EPI_RELU ? 1.0f / (1.0f - (float)p) : 1.0f;
    a.G = wants_g ? G : nullptr; a.ldg = ldg; a.part = db ? (float *)workspace : nullptr; a.part_ld = (d + 3) & ~3;
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = (n + PREP_ROWS - 1) / PREP_ROWS;
    const bool v4 = float4_rows(d, {{dY, lddy}, {a.Y, ldy}, {a.G, ldg}});
    a.chunks = v4 ? d / 4 : d;
    if (v4) hipLaunchKernelGGL(gcn_conv_prep_kernel<4>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    else hipLaunchKernelGGL(gcn_conv_prep_kernel<1>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    if (db) {
        hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), dim3((unsigned)((d + DB_COLS - 1) / DB_COLS)), dim3(DB_COLS * DB_SEGS), 0, st, blocks, d, a.part_ld,
                           (const float *)a.part, db);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}
