// ctgcn_vgrnn.hip — the decoder loss of the VGRNN baseline (reference baseline/vgrnn.py:402-413, metrics.py:154-161) without any
// [N, N] matrix.  With n rows, S the sum of the stored adjacency values, posw = (n^2 - S) / S and logits x_ij = z_i · z_j the
// reference's weighted BCE over the dense matrices equals
//
//   nll = [ sum_ij softplus(x_ij) + sum_stored a_e ((posw - 1) softplus(-x_e) - x_e) ] / (2 (n^2 - S))
//
//   dense     sum_ij softplus(x_ij) and dZ_i = 2 sum_j sigmoid(x_ij) z_j (x_ij and x_ji are one number) in one tiled pass over Z Z^T on
//             the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32).  A wave owns 32 rows I and walks every 32-column tile J: it forms
//             X^T = Z_J Z_I^T, so that its 16 accumulator registers hold column i = lane & 31 of the tile, which is the B operand of
//             the second product dZ_I^T += Z_J^T (2 sigmoid(X^T)) as it stands: no transpose, no LDS.  The k index of an MFMA step is
//             free as long as A and B agree, so a lane reads its operands of four steps as one float4 (k = 8 s + 4 (lane >> 5) + m).
//             Rows and columns beyond n are masked out of both sums (a zero row would add ln 2 per pair).  A lane's 16 softplus
//             values of a tile are added in fp32, the tiles in fp64, a wave's lanes by shuffles, the row tiles by one block in a
//             fixed order.
//   entries   per stored entry e = (i, j): x_e again as a 16-lane dot product, its loss term in fp64 and the coefficient
//             c_e = a_e (-(posw - 1) sigmoid(-x_e) - 1) = d term / d x_e.  dZ += C Z + C^T Z is then the plain row gather of
//             ctgcn_gcn.hip over the same CSR (and over the transposed one, whose coefficients a second call makes), long rows included.
// No atomics: every sum has a fixed order, so repeated launches are bit-identical.
//
// The model's three fused gathers (reference baseline/vgrnn.py:380-397, :497-508) on the ctgcn_gather.h scaffold.  The aggregation is
// linear, so the six convolutions of a graph-GRU step are two gathers and the two encoder heads one; a lane group owns a row and the
// hidden indices k, k + LPR, ... of it, gathers the k-th column of every segment of the wide source row (3 for the gates, 2 for the
// heads) and finishes the row in registers:
//   gates   [g_z | g_r | g_c] = Â U + b:  z = σ(g_z), r = σ(g_r), q = r ∘ h, c = g_c
//   blend   g = Â V:  h~ = tanh(c + g), h' = z ∘ h + (1 − z) ∘ h~
//   heads   [g_m | g_s] = Â S + b:  mean = g_m, std = softplus(g_s) (F.softplus's threshold 20), z = mean + noise ∘ std
// Long rows go through the piece kernel (plain partial sums of the whole wide row) and a final kernel that adds the pieces in order
// and runs the same finish.  The backward of each is one N x d pre-pass (epi_prep_kernel: the gradient G in front of the gather from the
// saved results, the gradients that do not pass the gather, and the bias gradient as per-block column sums added in block order by the
// scaffold's colsum_kernel), then the plain aggregation of G over the transposed CSR (ctgcn_gcn_conv_fwd_f32):
//   gates   G = [dz z (1 - z) | dq h r (1 - r) | dc], dh = dq r
//   blend   G = dh' (1 - z) (1 - h~^2) (also dc), dz = dh' (h - h~), dh = dh' z
//   heads   G = [dmean + dz | (dstd + dz noise) (1 - exp(-std))]: softplus' = sigmoid(pre) = 1 - exp(-std)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_reduce.h"
#include "ctgcn_try.h"

namespace {

typedef float f16 __attribute__((ext_vector_type(16)));

constexpr int TILE = 32;               // rows of a wave's row tile and columns of a column tile (ops.VAE_NLL_TILE)
constexpr int NLL_WAVES = 4;           // row tiles a block
constexpr int CHUNK = 128;             // columns of dZ a launch accumulates: 4 accumulator tiles of 16 registers
constexpr int KSTEPS = CHUNK / 8;      // float4 k-steps of the logits when d <= CHUNK: Z_I stays in registers
constexpr int ENT_LANES = 16;          // lanes across the feature row of one stored entry
constexpr int ENT_THREADS = 256;
constexpr int SUM_THREADS = 256;

struct NllArgs {
    int64_t n;
    int32_t d;
    const float *Z;
    int64_t ldz;
    float *dZ;              // null: the loss alone
    int64_t lddz;
    double *part;           // [row tiles] or null (a later column chunk: the loss is already counted)
    int32_t vec4;           // d and ldz multiples of 4, Z 16-byte aligned
    int32_t c0;             // first column of dZ this launch accumulates
};

// Z[row][k .. k + 3], zero beyond n rows or d columns
__device__ __forceinline__ f4 load4(const NllArgs &a, int64_t row, int k)
{
    f4 r = f4(0.f);
    if (row >= a.n || k >= a.d) return r;
    const float *p = a.Z + row * a.ldz + k;
    if (a.vec4) return *(const f4 *)p;                                // d % 4 == 0: k < d means k + 3 < d
    r.x = p[0];
    if (k + 1 < a.d) r.y = p[1];
    if (k + 2 < a.d) r.z = p[2];
    if (k + 3 < a.d) r.w = p[3];
    return r;
}

__device__ __forceinline__ f16 mfma4(f4 x, f4 y, f16 acc)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
    return acc;
}

// softplus(x) and sigmoid(x) from one exponential
__device__ __forceinline__ void softplus_sigmoid(float x, float &sp, float &sg)
{
    const float e = expf(-fabsf(x));
    sp = fmaxf(x, 0.f) + log1pf(e);
    const float inv = 1.f / (1.f + e);
    sg = x >= 0.f ? inv : e * inv;
}

// NT: accumulator tiles of dZ (columns c0 .. c0 + 32 NT); ZREG: d <= CHUNK, the wave's own rows stay in registers
template <int NT, bool ZREG>
__global__ __launch_bounds__(64 * NLL_WAVES) void nll_dense_kernel(const NllArgs a)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * NLL_WAVES + (threadIdx.x >> 6);
    const int64_t I0 = tile * TILE;
    if (I0 >= a.n) return;                                            // a whole wave; the kernel has no barrier
    const int64_t tiles = (a.n + TILE - 1) / TILE;
    const bool i_ok = I0 + r < a.n;
    const int ksteps = (a.d + 7) / 8;

    f4 zi[ZREG ? KSTEPS : 1];
    if (ZREG) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) zi[s] = load4(a, I0 + r, 8 * s + 4 * h);
    }
    f16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f16(0.f);
    double loss = 0.0;

    for (int64_t jt = 0; jt < tiles; ++jt) {
        const int64_t J0 = jt * TILE;
        // X^T[j][i]: A = Z_J (row = lane & 31), B = Z_I; register v of lane (r, h) is j = (v & 3) + 8 (v >> 2) + 4 h, i = r
        f16 x = f16(0.f);
        if (ZREG) {
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
                if (s < ksteps) x = mfma4(load4(a, J0 + r, 8 * s + 4 * h), zi[s], x);
        } else {
            for (int s = 0; s < ksteps; ++s) x = mfma4(load4(a, J0 + r, 8 * s + 4 * h), load4(a, I0 + r, 8 * s + 4 * h), x);
        }
        float ls = 0.f;
        f16 p;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const bool ok = i_ok && J0 + (v & 3) + 8 * (v >> 2) + 4 * h < a.n;
            float sp, sg;
            softplus_sigmoid(x[v], sp, sg);
            ls += ok ? sp : 0.f;
            p[v] = ok ? 2.f * sg : 0.f;
        }
        loss += (double)ls;
        if (!a.dZ) continue;
        // dZ_I^T[c][i] += sum_j Z_J[j][c] P^T[j][i]: step v takes the two j its register v holds, A = Z_J[j][c = lane & 31]
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = a.c0 + t * TILE + r;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t j = J0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                const float zj = (j < a.n && c < a.d) ? a.Z[j * a.ldz + c] : 0.f;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(zj, p[v], acc[t], 0, 0, 0);
            }
        }
    }
    if (a.part) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
        if (lane == 0) a.part[tile] = loss;
    }
    if (!a.dZ || !i_ok) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int c = a.c0 + t * TILE + (v & 3) + 8 * (v >> 2) + 4 * h;
            if (c < a.d) a.dZ[(I0 + r) * a.lddz + c] = acc[t][v];
        }
}

// out[0] = sum of part[0 .. count): thread t adds part[t], part[t + 256], ... in order, then the block's fixed tree
__global__ __launch_bounds__(SUM_THREADS) void nll_sum_kernel(int64_t count, const double *part, double *out)
{
    __shared__ double sh[SUM_THREADS];
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < count; k += SUM_THREADS) s += part[k];
    s = block_sum<SUM_THREADS>(s, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// 16 lanes an entry, 16 entries a block; the entry's row by bisection of row_ptr
__global__ __launch_bounds__(ENT_THREADS) void nll_entries_kernel(int64_t n, int64_t nnz, int32_t d, const int32_t *__restrict__ row_ptr,
                                                                 const int32_t *__restrict__ col, const float *__restrict__ val,
                                                                 const float *__restrict__ Z, int64_t ldz, double posw_m1,
                                                                 float *__restrict__ coef, double *part)
{
    __shared__ double sh[ENT_THREADS];
    const int lig = threadIdx.x & (ENT_LANES - 1);
    const int64_t e0 = (int64_t)blockIdx.x * (ENT_THREADS / ENT_LANES) + threadIdx.x / ENT_LANES;
    const bool live = e0 < nnz;
    const int32_t e = (int32_t)(live ? e0 : 0);                       // dead groups redo entry 0 and write nothing
    int64_t lo = 0, hi = n;                                           // row_ptr[lo] <= e < row_ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int64_t j = col[e];
    const bool ok = live && j >= 0 && j < n;
    const float *zi = Z + lo * ldz, *zj = Z + (ok ? j : 0) * ldz;
    float dot = 0.f;
    for (int c = lig; c < d; c += ENT_LANES) dot = fmaf(zi[c], zj[c], dot);
#pragma unroll
    for (int o = ENT_LANES / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, ENT_LANES);
    float sp, sg;
    softplus_sigmoid(-dot, sp, sg);
    const double w = (double)val[e];
    double term = 0.0;
    if (ok && lig == 0) {
        term = w * (posw_m1 * (double)sp - (double)dot);
        coef[e] = (float)(w * (-posw_m1 * (double)sg - 1.0));
    } else if (live && lig == 0) {
        coef[e] = 0.f;
    }
    if (part) {                                                       // block-uniform
        const double s = block_sum<ENT_THREADS>(term, sh);
        if (threadIdx.x == 0) part[blockIdx.x] = s;
    }
}

// ------------------------------------------------------------------------------------------------ the model's fused gathers
constexpr int MODE_GATES = 0, MODE_BLEND = 1, MODE_HEADS = 2;
template <int MODE> struct segs_of { static constexpr int value = MODE == MODE_GATES ? 3 : MODE == MODE_HEADS ? 2 : 1; };

struct EpiArgs {
    int64_t n;
    int32_t d, w;           // width of the gathered row, and of one segment of it (the hidden or the output width)
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    const float *src;       // [n, d]: U, V or S
    int64_t ldsrc;
    const float *bias;      // [d] or null
    const float *a, *b, *c; // [n, w] operands.  gates: a = h; blend: a = c, b = z, c = h; heads: a = noise
    int64_t lda, ldb, ldc;
    float *o0, *o1, *o2, *o3;   // [n, w], row stride w.  gates: z, r, q, c; blend: h', h~; heads: mean, std, z
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t chunks;         // ceil(w / VEC)
    int32_t max_pieces;
    int32_t part_ld;        // d rounded up to 4
    float *part;            // [n_long][max_pieces][part_ld]
};

__device__ __forceinline__ float sigmoid1(float x)
{
    const float e = expf(-fabsf(x));
    const float inv = 1.f / (1.f + e);
    return x >= 0.f ? inv : e * inv;
}

// the finished sums t[segment] of hidden index k of a row -> the row's results
template <int MODE>
__device__ __forceinline__ void finish(const EpiArgs &a, int64_t row, int k, const float *t)
{
    const int64_t o = row * a.w + k;
    if (MODE == MODE_GATES) {
        float gz = t[0], gr = t[1], gc = t[2];
        if (a.bias) {
            gz += a.bias[k];
            gr += a.bias[a.w + k];
            gc += a.bias[2 * a.w + k];
        }
        const float r = sigmoid1(gr);
        a.o0[o] = sigmoid1(gz);
        a.o1[o] = r;
        a.o2[o] = r * a.a[row * a.lda + k];
        a.o3[o] = gc;
    } else if (MODE == MODE_BLEND) {
        const float ht = tanhf(t[0] + a.a[row * a.lda + k]);
        const float z = a.b[row * a.ldb + k], h = a.c[row * a.ldc + k];
        a.o1[o] = ht;
        a.o0[o] = z * h + (1.f - z) * ht;
    } else {
        float m = t[0], g = t[1];
        if (a.bias) {
            m += a.bias[k];
            g += a.bias[a.w + k];
        }
        const float sd = g > 20.f ? g : log1pf(expf(g));
        a.o0[o] = m;
        a.o1[o] = sd;
        a.o2[o] = m + a.a[row * a.lda + k] * sd;
    }
}

__device__ __forceinline__ float comp(f4 v, int m) { return v[m]; }
__device__ __forceinline__ float comp(float v, int) { return v; }

// P[s] = sum_e val[e] src[col[e]][s w + foff ..] over the entries [start, end) of a row, by the row's LPR lanes (ctgcn_gcn.hip's row_sum
// with SEGS columns per entry)
template <int VEC, int LPR, int SEGS>
__device__ __forceinline__ void row_sums(const EpiArgs &a, int start, int end, int lig, int64_t foff, typename vec_of<VEC>::type *P)
{
    using V = typename vec_of<VEC>::type;
    constexpr int UU = SEGS == 1 ? 4 : 2;                             // gathered rows in flight per lane group
#pragma unroll
    for (int s = 0; s < SEGS; ++s) P[s] = V(0.f);
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
        for (; j + UU <= cnt; j += UU) {
            V xv[UU][SEGS];
            float wj[UU];
#pragma unroll
            for (int u = 0; u < UU; ++u) {
                const int cj = __shfl(c, j + u, LPR);
                wj[u] = __shfl(w, j + u, LPR);
                const float *p = a.src + (int64_t)cj * a.ldsrc + foff;
#pragma unroll
                for (int s = 0; s < SEGS; ++s) xv[u][s] = *(const V *)(p + (int64_t)s * a.w);
            }
#pragma unroll
            for (int u = 0; u < UU; ++u)
#pragma unroll
                for (int s = 0; s < SEGS; ++s) P[s] = vfma(wj[u], xv[u][s], P[s]);
        }
        for (; j < cnt; ++j) {
            const int cj = __shfl(c, j, LPR);
            const float w1 = __shfl(w, j, LPR);
            const float *p = a.src + (int64_t)cj * a.ldsrc + foff;
#pragma unroll
            for (int s = 0; s < SEGS; ++s) P[s] = vfma(w1, *(const V *)(p + (int64_t)s * a.w), P[s]);
        }
    }
}

// every row that is not long
template <int VEC, int LPR, int MODE>
__global__ __launch_bounds__(256) void epi_row_kernel(const EpiArgs a)
{
    using V = typename vec_of<VEC>::type;
    constexpr int SEGS = segs_of<MODE>::value;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    const int start = a.row_ptr[row], end = a.row_ptr[row + 1];
    if (a.n_long > 0 && end - start > a.long_thresh) return;         // long row: epi_piece_kernel + epi_final_kernel
    for (int p0 = 0; p0 < a.chunks; p0 += LPR) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;            // dead lanes read chunk 0 (valid memory) and never store
        V P[SEGS];
        row_sums<VEC, LPR, SEGS>(a, start, end, lig, foff, P);
        if (!live) continue;
#pragma unroll
        for (int m = 0; m < VEC; ++m) {
            float t[SEGS];
#pragma unroll
            for (int s = 0; s < SEGS; ++s) t[s] = comp(P[s], m);
            finish<MODE>(a, row, (int)foff + m, t);
        }
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of long row i, all d columns, into part[i][p]
template <int VEC>
__global__ __launch_bounds__(PIECE_THREADS) void epi_piece_kernel(const EpiArgs a)
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
    const int chunks = (a.d + VEC - 1) / VEC;

    for (int p0 = 0; p0 < chunks; p0 += PIECE_LANES) {
        const int ch = p0 + lig;
        const bool live = ch < chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
        for (int e = lo + g; e < hi; e += PIECE_GROUPS) P = vfma(a.val[e], *(const V *)(a.src + (int64_t)a.col[e] * a.ldsrc + foff), P);
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

// one wave per long row: the pieces in piece order, then the row's finish
template <int MODE>
__global__ __launch_bounds__(64) void epi_final_kernel(const EpiArgs a)
{
    constexpr int SEGS = segs_of<MODE>::value;
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    for (int k = threadIdx.x; k < a.w; k += 64) {
        float t[SEGS];
#pragma unroll
        for (int s = 0; s < SEGS; ++s) {
            const int c = s * a.w + k;
            float v = src[c];
            for (int p = 1; p < np; ++p) v += src[(int64_t)p * a.part_ld + c];
            t[s] = v;
        }
        finish<MODE>(a, row, k, t);
    }
}

template <int VEC, int MODE>
int launch_epi(EpiArgs a, hipStream_t st)
{
    a.chunks = (a.w + VEC - 1) / VEC;
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((epi_row_kernel<VEC, decltype(lpr)::value, MODE>), grid, dim3(256), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL((epi_piece_kernel<VEC>), grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL((epi_final_kernel<MODE>), grid, dim3(64), 0, st, a); });
}

// the checks the three entry points share; a.src, a.ldsrc and the operands are set by the caller.  n == 0 launches nothing.
template <int MODE>
int run_epi(EpiArgs &a, const char *what, int64_t n, int32_t w, const int32_t *row_ptr, const int32_t *col, const float *val,
            const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    constexpr int SEGS = segs_of<MODE>::value;
    if (n < 0 || n > INT32_MAX || w < 1 || w > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and 1 <= width < 2^29");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val || !a.src || !a.a || !a.o0 || !a.o1 || (MODE != MODE_BLEND && !a.o2) || (MODE == MODE_GATES && !a.o3) ||
        (MODE == MODE_BLEND && (!a.b || !a.c)))
        return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.n = n; a.w = w; a.d = SEGS * w; a.row_ptr = row_ptr; a.col = col; a.val = val;
    if (a.ldsrc < a.d || a.lda < w || (MODE == MODE_BLEND && (a.ldb < w || a.ldc < w))) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below the width");
    a.part_ld = (a.d + 3) & ~3;
    if (int rc = set_long_rows(a, what, long_rows, n_long, long_threshold, a.part_ld, workspace, workspace_bytes,
                               "long rows need a 16-byte aligned workspace of at least n_long * round_up(gathered width, 4) * 4 bytes (one piece per row)"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // float4 rows: every segment starts on a float4 of the source row
    return (w % 4 == 0 && a.ldsrc % 4 == 0 && ctgcn_aligned16(a.src)) ? launch_epi<4, MODE>(a, st) : launch_epi<1, MODE>(a, st);
}

// ------------------------------------------------------------------------------------------------ their backward pre-pass
struct PrepEpi {
    int64_t n;
    int32_t w, d;
    const float *g0, *g1, *g2;      // incoming gradients [n, w], null = zero.  gates: dz, dq, dc; blend: dh'; heads: dmean, dstd, dz
    int64_t ldg0, ldg1, ldg2;
    const float *s0, *s1, *s2;      // saved [n, w].  gates: z, r, h; blend: z, h, h~; heads: std, noise
    int64_t lds0, lds1, lds2;
    float *G;                       // [n, d]
    int64_t ldG;
    float *x0, *x1;                 // [n, w], row stride w.  gates: dh; blend: dz, dh
    float *part;                    // [blocks][part_ld] or null
    int32_t part_ld;
};

__device__ __forceinline__ float at(const float *p, int64_t row, int64_t ld, int k) { return p ? p[row * ld + k] : 0.f; }

// PREP_ROWS rows a block; wave v takes the block's rows v, v + 4, ..., its lanes lie across the hidden index
template <int MODE>
__global__ __launch_bounds__(64 * PREP_WAVES) void epi_prep_kernel(const PrepEpi a)
{
    constexpr int SEGS = segs_of<MODE>::value;
    __shared__ float sm[PREP_WAVES][SEGS][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    for (int k0 = 0; k0 < a.w; k0 += 64) {
        const int k = k0 + lane;
        const bool live = k < a.w;
        float acc[SEGS];
#pragma unroll
        for (int s = 0; s < SEGS; ++s) acc[s] = 0.f;
        if (live) {
            for (int r = wv; r < PREP_ROWS && row0 + r < a.n; r += PREP_WAVES) {
                const int64_t row = row0 + r;
                float g[SEGS];
                if (MODE == MODE_GATES) {
                    const float z = a.s0[row * a.lds0 + k], rr = a.s1[row * a.lds1 + k], h = a.s2[row * a.lds2 + k];
                    const float dq = at(a.g1, row, a.ldg1, k);
                    g[0] = at(a.g0, row, a.ldg0, k) * z * (1.f - z);
                    g[1] = dq * h * rr * (1.f - rr);
                    g[2] = at(a.g2, row, a.ldg2, k);
                    a.x0[row * a.w + k] = dq * rr;
                } else if (MODE == MODE_BLEND) {
                    const float z = a.s0[row * a.lds0 + k], h = a.s1[row * a.lds1 + k], ht = a.s2[row * a.lds2 + k];
                    const float dh = a.g0[row * a.ldg0 + k];
                    g[0] = dh * (1.f - z) * (1.f - ht * ht);
                    a.x0[row * a.w + k] = dh * (h - ht);
                    a.x1[row * a.w + k] = dh * z;
                } else {
                    const float sd = a.s0[row * a.lds0 + k], nz = a.s1[row * a.lds1 + k];
                    const float dz = at(a.g2, row, a.ldg2, k);
                    g[0] = at(a.g0, row, a.ldg0, k) + dz;
                    g[1] = (at(a.g1, row, a.ldg1, k) + dz * nz) * -expm1f(-sd);
                }
#pragma unroll
                for (int s = 0; s < SEGS; ++s) {
                    a.G[row * a.ldG + (int64_t)s * a.w + k] = g[s];
                    acc[s] += g[s];
                }
            }
        }
        if (a.part) {                                                 // block-uniform
#pragma unroll
            for (int s = 0; s < SEGS; ++s) sm[wv][s][lane] = acc[s];
            __syncthreads();
            if (wv == 0 && live) {
#pragma unroll
                for (int s = 0; s < SEGS; ++s) {
                    float t = sm[0][s][lane];
#pragma unroll
                    for (int v = 1; v < PREP_WAVES; ++v) t += sm[v][s][lane];
                    a.part[(int64_t)blockIdx.x * a.part_ld + (int64_t)s * a.w + k] = t;
                }
            }
            __syncthreads();
        }
    }
}

template <int MODE>
int run_prep(PrepEpi &a, const char *what, float *db, void *workspace, size_t workspace_bytes, void *stream)
{
    constexpr int SEGS = segs_of<MODE>::value;
    a.d = SEGS * a.w;
    a.part_ld = (a.d + 3) & ~3;
    const int64_t blocks = (a.n + PREP_ROWS - 1) / PREP_ROWS;
    if (!a.s0 || !a.s1 || (MODE != MODE_HEADS && !a.s2) || !a.G || (MODE != MODE_HEADS && !a.x0) || (MODE == MODE_BLEND && (!a.x1 || !a.g0)))
        return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if ((a.g0 && a.ldg0 < a.w) || (a.g1 && a.ldg1 < a.w) || (a.g2 && a.ldg2 < a.w) || a.lds0 < a.w || a.lds1 < a.w || (a.s2 && a.lds2 < a.w) ||
        a.ldG < a.d)
        return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below the width");
    if (db && (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < (size_t)blocks * a.part_ld * sizeof(float)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "a bias gradient needs a 16-byte aligned workspace of ctgcn_gcn_conv_prep_workspace_bytes(n, gathered width) bytes");
    a.part = db ? (float *)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((epi_prep_kernel<MODE>), dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    if (db) {
        hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), dim3((unsigned)((a.d + DB_COLS - 1) / DB_COLS)), dim3(DB_COLS * DB_SEGS), 0, st, blocks, a.d,
                           a.part_ld, (const float *)a.part, db);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

int64_t dense_tiles(int64_t n) { return (n + TILE - 1) / TILE; }
int64_t entry_blocks(int64_t nnz) { return (nnz + ENT_THREADS / ENT_LANES - 1) / (ENT_THREADS / ENT_LANES); }

bool bad_workspace(const void *ws, size_t have, size_t need) { return need && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7) || have < need); }

}  // namespace

extern "C" int32_t ctgcn_vae_nll_tile(void) { return TILE; }

extern "C" size_t ctgcn_vae_nll_workspace_bytes(int64_t n, int64_t nnz)
{
    if (n < 0 || nnz < 0) return 0;
    const int64_t a = dense_tiles(n), b = entry_blocks(nnz);
    return (size_t)(a > b ? a : b) * sizeof(double);
}

extern "C" int ctgcn_vae_nll_dense_f32(int64_t n, int32_t d, const float *Z, int64_t ldz, float *dZ, int64_t lddz, double *loss,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "vae_nll_dense";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (!loss) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return CTGCN_OK;
    if (!Z) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (ldz < d || (dZ && lddz < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    const int64_t tiles = dense_tiles(n);
    if (bad_workspace(workspace, workspace_bytes, (size_t)tiles * sizeof(double)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 8-byte aligned and hold ctgcn_vae_nll_workspace_bytes() bytes");
    NllArgs a{};
    a.n = n; a.d = d; a.Z = Z; a.ldz = ldz; a.dZ = dZ; a.lddz = lddz; a.part = (double *)workspace;
    a.vec4 = ctgcn_can_vec4(d, Z, ldz);
    const dim3 grid((unsigned)((tiles + NLL_WAVES - 1) / NLL_WAVES)), block(64 * NLL_WAVES);
    if (d <= TILE) hipLaunchKernelGGL((nll_dense_kernel<1, true>), grid, block, 0, st, a);
    else if (d <= 2 * TILE) hipLaunchKernelGGL((nll_dense_kernel<2, true>), grid, block, 0, st, a);
    else if (d <= CHUNK) hipLaunchKernelGGL((nll_dense_kernel<4, true>), grid, block, 0, st, a);
    else {
        // wider than the accumulators: one launch per 128 columns of dZ, each forming the logits again; the first counts the loss
        for (int32_t c0 = 0; c0 < (dZ ? d : 1); c0 += CHUNK) {
            a.c0 = c0;
            a.part = c0 ? nullptr : (double *)workspace;
            hipLaunchKernelGGL((nll_dense_kernel<4, false>), grid, block, 0, st, a);
            CTGCN_TRY(hipGetLastError());
        }
    }
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(nll_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, st, tiles, (const double *)workspace, loss);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_vae_nll_entries_f32(int64_t n, int64_t nnz, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val,
                                         const float *Z, int64_t ldz, double posw_m1, float *coef, double *loss, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    const char *what = "vae_nll_entries";
    if (n < 0 || n > INT32_MAX || nnz < 0 || nnz > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n, nnz < 2^31 and d >= 1");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || nnz == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val || !Z || !coef) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (ldz < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    const int64_t blocks = entry_blocks(nnz);
    if (loss && bad_workspace(workspace, workspace_bytes, (size_t)blocks * sizeof(double)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 8-byte aligned and hold ctgcn_vae_nll_workspace_bytes() bytes");
    double *part = loss ? (double *)workspace : nullptr;
    hipLaunchKernelGGL(nll_entries_kernel, dim3((unsigned)blocks), dim3(ENT_THREADS), 0, st, n, nnz, d, row_ptr, col, val, Z, ldz, posw_m1,
                       coef, part);
    CTGCN_TRY(hipGetLastError());
    if (loss) {
        hipLaunchKernelGGL(nll_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, st, blocks, (const double *)part, loss);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

extern "C" int ctgcn_ggru_gates_fwd_f32(int64_t n, int32_t hid, const int32_t *row_ptr, const int32_t *col, const float *val, const float *U,
                                        int64_t ldu, const float *bias, const float *h, int64_t ldh, float *z, float *r, float *q, float *c,
                                        const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    EpiArgs a{};
    a.src = U; a.ldsrc = ldu; a.bias = bias; a.a = h; a.lda = ldh; a.o0 = z; a.o1 = r; a.o2 = q; a.o3 = c;
    return run_epi<MODE_GATES>(a, "ggru_gates_fwd", n, hid, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_ggru_blend_fwd_f32(int64_t n, int32_t hid, const int32_t *row_ptr, const int32_t *col, const float *val, const float *V,
                                        int64_t ldv, const float *c, int64_t ldc, const float *z, int64_t ldz, const float *h, int64_t ldh,
                                        float *h_new, float *h_tilde, const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    EpiArgs a{};
    a.src = V; a.ldsrc = ldv; a.a = c; a.lda = ldc; a.b = z; a.ldb = ldz; a.c = h; a.ldc = ldh; a.o0 = h_new; a.o1 = h_tilde;
    return run_epi<MODE_BLEND>(a, "ggru_blend_fwd", n, hid, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_vgrnn_heads_fwd_f32(int64_t n, int32_t out, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                         int64_t lds, const float *bias, const float *noise, int64_t ldnoise, float *mean, float *std_out,
                                         float *z, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    EpiArgs a{};
    a.src = S; a.ldsrc = lds; a.bias = bias; a.a = noise; a.lda = ldnoise; a.o0 = mean; a.o1 = std_out; a.o2 = z;
    return run_epi<MODE_HEADS>(a, "vgrnn_heads_fwd", n, out, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_vgrnn_bwd_prep_f32(int32_t mode, int64_t n, int32_t width, const float *g0, int64_t ldg0, const float *g1, int64_t ldg1,
                                        const float *g2, int64_t ldg2, const float *s0, int64_t lds0, const float *s1, int64_t lds1,
                                        const float *s2, int64_t lds2, float *G, int64_t ldG, float *x0, float *x1, float *db, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    const char *what = "vgrnn_bwd_prep";
    if (mode != MODE_GATES && mode != MODE_BLEND && mode != MODE_HEADS) return ctgcn_fail(CTGCN_E_INVALID, what, "mode must be 0 (gates), 1 (blend) or 2 (heads)");
    if (n < 0 || n > INT32_MAX || width < 1 || width > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and 1 <= width < 2^29");
    if (n == 0) return CTGCN_OK;
    PrepEpi a{};
    a.n = n; a.w = width; a.g0 = g0; a.ldg0 = ldg0; a.g1 = g1; a.ldg1 = ldg1; a.g2 = g2; a.ldg2 = ldg2;
    a.s0 = s0; a.lds0 = lds0; a.s1 = s1; a.lds1 = lds1; a.s2 = s2; a.lds2 = lds2; a.G = G; a.ldG = ldG; a.x0 = x0; a.x1 = x1;
    if (mode == MODE_GATES) return run_prep<MODE_GATES>(a, what, db, workspace, workspace_bytes, stream);
    if (mode == MODE_BLEND) return run_prep<MODE_BLEND>(a, what, nullptr, nullptr, 0, stream);
    return run_prep<MODE_HEADS>(a, what, db, workspace, workspace_bytes, stream);
}
