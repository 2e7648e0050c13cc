// ctgcn_sim.hip — similarity-prediction evaluation (reference evaluation/similarity_prediction.py) on the GPU.
//
//   - sim_step_kernel: one step S <- c·A·S + I of Leicht–Holme–Newman vertex similarity on a column panel.  Each output entry is one
//     thread's fp64 sum over its CSR row in CSR order, acc = acc + a_ij·x_j from +0.0, then c·acc + δ_ij: the operations and their
//     order of scipy's csr_matvecs, never contracted to FMA (`fp contract(off)` below), so S is bit-identical to the reference's.
//     Columns are independent, so every step of a panel runs before the next panel starts; the panel's two ping-pong buffers are
//     sized by ctgcn_sim_panel_cols to stay inside the Infinity Cache, and the last step writes the panel into S directly.
//   - sim_sym_kernel / sim_norm_kernel / sim_coo_kernel: the finish over the m x m block: (S + Sᵀ)/2 - I in place one pair of
//     transposed 32 x 32 tiles at a time through LDS with min/max tile partials, then (S - min)/(max - min) and the 1e-6 threshold
//     with per-row non-zero counts, then the row-major COO of the original vertex ids.
//   - sim_gram_kernel / sim_scale_kernel / sim_np_chunk_kernel / sim_rank_kernel / sim_corr_kernel: the predictor: E Eᵀ over the
//     kept rows (each unordered pair once, mirrored), the reference's min-max and sum normalisations (the sum in numpy's order, bit for
//     bit: the correlation moves by 1e-9 with the sum's last bit), and the average-rank Spearman sums.
// No float atomics: every reduction is per-block partials summed in a fixed order, and the block counts depend on the sizes alone,
// so repeated calls are bit-identical and the series does not depend on the panel width.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "ctgcn_reduce.h"
#include "ctgcn_try.h"

#pragma clang fp contract(off)

namespace {

constexpr int ST = 256;                          // series / elementwise block
constexpr int TT = 32;                           // finish / Gram tile edge
constexpr int RB = 256;                          // reduction block
constexpr int MAX_RED_BLOCKS = 1024;             // partial blocks of a reduction over N values
constexpr int64_t MIN_PER_BLOCK = 4096;
constexpr size_t CACHE_BUDGET = (size_t)200 << 20;   // panel buffers + A kept under the 256 MiB Infinity Cache

__host__ __device__ __forceinline__ int64_t red_blocks(int64_t N)
{
    const int64_t b = (N + MIN_PER_BLOCK - 1) / MIN_PER_BLOCK;
    return b < 1 ? 1 : (b < MAX_RED_BLOCKS ? b : MAX_RED_BLOCKS);
}

// ---------------------------------------------------------------- series

// X[i*ld + j] = (i == j0 + j) for j < w
__global__ __launch_bounds__(ST) void sim_eye_kernel(int64_t m, int64_t w, int64_t j0, double *__restrict__ X, int64_t ld)
{
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= m * w) return;
    const int64_t i = t / w, j = t - i * w;
    X[i * ld + j] = (i == j0 + j) ? 1.0 : 0.0;
}

// Y[i*ldy + j] = c·Σ_e val[e]·X[col[e]*w + j] + (i == j0 + j), the sum in CSR order from +0.0, non-fused
__global__ __launch_bounds__(ST) void sim_step_kernel(int64_t m, int64_t w, int64_t j0, const int32_t *__restrict__ row_ptr,
                                                      const int32_t *__restrict__ col, const double *__restrict__ val, double c,
                                                      const double *__restrict__ X, double *__restrict__ Y, int64_t ldy)
{
    const int64_t t = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (t >= m * w) return;
    const int64_t i = t / w, j = t - i * w;
    const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
    double acc = 0.0;
    int e = e0;
    for (; e + 4 <= e1; e += 4) {        // four gathers in flight, summed in order
        const double a0 = val[e], a1 = val[e + 1], a2 = val[e + 2], a3 = val[e + 3];
        const double x0 = X[(int64_t)col[e] * w + j], x1 = X[(int64_t)col[e + 1] * w + j];
        const double x2 = X[(int64_t)col[e + 2] * w + j], x3 = X[(int64_t)col[e + 3] * w + j];
        acc = acc + a0 * x0;
        acc = acc + a1 * x1;
        acc = acc + a2 * x2;
        acc = acc + a3 * x3;
    }
    for (; e < e1; ++e) acc = acc + val[e] * X[(int64_t)col[e] * w + j];
    Y[i * ldy + j] = c * acc + ((i == j0 + j) ? 1.0 : 0.0);
}

// ---------------------------------------------------------------- finish

// Tile pair (bi, bj), bi <= bj: S <- (S + Sᵀ)/2 - I on both tiles; part[(bi*T + bj)*2 + {0, 1}] = min, max of the pair's new values
// (blocks with bi > bj write the neutral pair)
__global__ __launch_bounds__(ST) void sim_sym_kernel(int64_t m, int64_t T, double *__restrict__ S, double *__restrict__ part)
{
    __shared__ double A[TT][TT + 1], B[TT][TT + 1];
    __shared__ double rmin[ST / 64], rmax[ST / 64];
    const int64_t bi = blockIdx.y, bj = blockIdx.x;
    const int tx = threadIdx.x & (TT - 1), ty = threadIdx.x / TT;      // 32 x 8
    double lo = __builtin_inf(), hi = -__builtin_inf();
    if (bi <= bj) {
        for (int r = ty; r < TT; r += ST / TT) {
            const int64_t i = bi * TT + r, j = bj * TT + tx;
            if (i < m && j < m) A[r][tx] = S[i * m + j];
            const int64_t i2 = bj * TT + r, j2 = bi * TT + tx;
            if (i2 < m && j2 < m) B[r][tx] = S[i2 * m + j2];
        }
        __syncthreads();
        for (int r = ty; r < TT; r += ST / TT) {
            const int64_t i = bi * TT + r, j = bj * TT + tx;
            if (i < m && j < m) {
                double v = (A[r][tx] + B[tx][r]) / 2.0;
                v = v - ((i == j) ? 1.0 : 0.0);
                S[i * m + j] = v;
                lo = fmin(lo, v);
                hi = fmax(hi, v);
            }
            const int64_t i2 = bj * TT + r, j2 = bi * TT + tx;
            if (bi != bj && i2 < m && j2 < m) {
                const double v = (B[r][tx] + A[tx][r]) / 2.0;
                S[i2 * m + j2] = v;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        rmin[wv] = lo;
        rmax[wv] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < ST / 64; ++k) {
            lo = fmin(lo, rmin[k]);
            hi = fmax(hi, rmax[k]);
        }
        part[(bi * T + bj) * 2] = fmin(lo, rmin[0]);
        part[(bi * T + bj) * 2 + 1] = fmax(hi, rmax[0]);
    }
}

// stats[0..1] = min, max over `count` (min, max) partials, and over 0 when pad_zero
__global__ __launch_bounds__(RB) void sim_minmax_reduce_kernel(int64_t count, const double *__restrict__ part, int pad_zero,
                                                               double *__restrict__ stats)
{
    __shared__ double smin[RB], smax[RB];
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int64_t k = threadIdx.x; k < count; k += RB) {
        lo = fmin(lo, part[2 * k]);
        hi = fmax(hi, part[2 * k + 1]);
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = RB / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = pad_zero ? fmin(smin[0], 0.0) : smin[0];
        stats[1] = pad_zero ? fmax(smax[0], 0.0) : smax[0];
    }
}

// row i (one block): S <- (S - min) / (max - min), zero below eps; row_nnz[i] = the entries left non-zero (NaN counts)
__global__ __launch_bounds__(ST) void sim_norm_kernel(int64_t m, double *__restrict__ S, const double *__restrict__ stats, double eps,
                                                      int64_t *__restrict__ row_nnz)
{
    const int64_t i = blockIdx.x;
    const double mn = stats[0], range = stats[1] - stats[0];
    double *row = S + i * m;
    int64_t cnt = 0;
    for (int64_t j0 = 0; j0 < m; j0 += ST) {
        const int64_t j = j0 + threadIdx.x;
        int nz = 0;
        if (j < m) {
            double v = (row[j] - mn) / range;
            if (v < eps) v = 0.0;
            row[j] = v;
            nz = v != 0.0;
        }
        cnt += __syncthreads_count(nz);
    }
    if (threadIdx.x == 0) row_nnz[i] = cnt;
}

// row i (one block): its non-zeros in column order at [row_off[i], ...): (ids[i], ids[j], S[i, j])
__global__ __launch_bounds__(ST) void sim_coo_kernel(int64_t m, const double *__restrict__ S, const int64_t *__restrict__ row_off,
                                                     const int64_t *__restrict__ ids, int32_t *__restrict__ row_out,
                                                     int32_t *__restrict__ col_out, double *__restrict__ data_out)
{
    __shared__ int wcnt[ST / 64];
    const int64_t i = blockIdx.x;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double *row = S + i * m;
    const int32_t rid = (int32_t)ids[i];
    int64_t base = row_off[i];
    for (int64_t j0 = 0; j0 < m; j0 += ST) {
        const int64_t j = j0 + threadIdx.x;
        const double v = j < m ? row[j] : 0.0;
        const bool nz = v != 0.0;
        const unsigned long long bal = __ballot(nz);
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int64_t pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) pos += wcnt[k];
        if (nz) {
            row_out[pos] = rid;
            col_out[pos] = (int32_t)ids[j];
            data_out[pos] = v;
        }
        for (int k = 0; k < ST / 64; ++k) base += wcnt[k];
        __syncthreads();
    }
}

// ---------------------------------------------------------------- predictor

// out[a, b] = out[b, a] = Σ_k E[rows[a], k]·E[rows[b], k] (fp64, k in order) for the tile pair (ta, tb), ta <= tb
template <typename T>
__global__ __launch_bounds__(ST) void sim_gram_kernel(int64_t m, int d, const T *__restrict__ E, int64_t lde,
                                                      const int64_t *__restrict__ rows, double *__restrict__ out)
{
    __shared__ double Ea[TT][TT + 1], Eb[TT][TT + 1];
    const int64_t ta = blockIdx.y, tb = blockIdx.x;
    if (ta > tb) return;
    const int tx = threadIdx.x & (TT - 1), ty = threadIdx.x / TT;
    double acc[TT / (ST / TT)] = {};
    for (int k0 = 0; k0 < d; k0 += TT) {
        for (int r = ty; r < TT; r += ST / TT) {
            const int64_t a = ta * TT + r, b = tb * TT + r;
            const int k = k0 + tx;
            Ea[r][tx] = (a < m && k < d) ? (double)E[rows[a] * lde + k] : 0.0;
            Eb[r][tx] = (b < m && k < d) ? (double)E[rows[b] * lde + k] : 0.0;
        }
        __syncthreads();
        const int kn = d - k0 < TT ? d - k0 : TT;
        for (int k = 0; k < kn; ++k) {
            const double eb = Eb[tx][k];
#pragma unroll
            for (int q = 0; q < TT / (ST / TT); ++q) acc[q] = fma(Ea[ty + q * (ST / TT)][k], eb, acc[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < TT / (ST / TT); ++q) {
        const int64_t a = ta * TT + ty + q * (ST / TT), b = tb * TT + tx;
        if (a < m && b < m) {
            out[a * m + b] = acc[q];
            if (ta != tb) out[b * m + a] = acc[q];
        }
    }
}

// part[b*2 + {0, 1}] = min, max of x over block b's grid-stride share
__global__ __launch_bounds__(RB) void sim_minmax_kernel(int64_t N, const double *__restrict__ x, double *__restrict__ part)
{
    __shared__ double smin[RB], smax[RB];
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x; k < N; k += (int64_t)gridDim.x * RB) {
        lo = fmin(lo, x[k]);
        hi = fmax(hi, x[k]);
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = RB / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = smin[0];
        part[2 * blockIdx.x + 1] = smax[0];
    }
}

// x <- (x - min) / (max - min) (stats[0..1])
__global__ __launch_bounds__(RB) void sim_scale_kernel(int64_t N, double *__restrict__ x, const double *__restrict__ stats)
{
    const double mn = stats[0], range = stats[1] - stats[0];
    for (int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x; k < N; k += (int64_t)gridDim.x * RB) x[k] = (x[k] - mn) / range;
}

// numpy's float64 sum, bit for bit: the array is reduced in chunks of NP_BUF elements (the ufunc buffer), each summed pairwise
// (halves cut at multiples of 8 down to blocks of at most 128, which use 8 running sums), and the chunk sums are added in order
// from 0.0.  A chunk per thread; the tree walk keeps an explicit stack.
constexpr int64_t NP_BUF = 8192;
constexpr int64_t NP_BLOCK = 128;

__device__ double np_block_sum(const double *__restrict__ a, int64_t n)
{
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r = r + a[i];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a[i];
    return res;
}

__device__ double np_pairwise_sum(const double *__restrict__ a, int64_t n)
{
    int64_t lo_s[16], n_s[16];
    double left_s[16];
    int right_s[16];
    int sp = 0;
    lo_s[0] = 0;
    n_s[0] = n;
    right_s[0] = 0;
    for (;;) {
        if (n_s[sp] > NP_BLOCK) {                  // descend into the left half
            int64_t h = n_s[sp] / 2;
            h -= h % 8;
            lo_s[sp + 1] = lo_s[sp];
            n_s[sp + 1] = h;
            right_s[sp + 1] = 0;
            ++sp;
            continue;
        }
        double ret = np_block_sum(a + lo_s[sp], n_s[sp]);
        for (;;) {
            if (sp == 0) return ret;
            --sp;
            if (!right_s[sp + 1]) {                // the left half is done: keep it, then the right half
                left_s[sp] = ret;
                int64_t h = n_s[sp] / 2;
                h -= h % 8;
                lo_s[sp + 1] = lo_s[sp] + h;
                n_s[sp + 1] = n_s[sp] - h;
                right_s[sp + 1] = 1;
                ++sp;
                break;
            }
            ret = left_s[sp] + ret;               // both halves done
        }
    }
}

__global__ __launch_bounds__(RB) void sim_np_chunk_kernel(int64_t N, const double *__restrict__ x, double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * RB + threadIdx.x, lo = c * NP_BUF;
    if (lo >= N) return;
    part[c] = np_pairwise_sum(x + lo, N - lo < NP_BUF ? N - lo : NP_BUF);
}

__global__ void sim_np_total_kernel(int64_t chunks, const double *__restrict__ part, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int64_t c = 0; c < chunks; ++c) s = s + part[c];
    *out = s;
}

// out[0..k) = the sums of the `count` k-vectors of part (k <= 3), in a fixed order
__global__ __launch_bounds__(RB) void sim_sum_reduce_kernel(int64_t count, int k, const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double sh[RB];
    for (int q = 0; q < k; ++q) {
        double s = 0.0;
        for (int64_t b = threadIdx.x; b < count; b += RB) s = s + part[b * k + q];
        const double r = block_sum<RB>(s, sh);
        if (threadIdx.x == 0) out[q] = r;
    }
}

__global__ __launch_bounds__(RB) void sim_div_kernel(int64_t N, double *__restrict__ x, const double *__restrict__ stats)
{
    const double s = stats[2];
    for (int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x; k < N; k += (int64_t)gridDim.x * RB) x[k] = x[k] / s;
}

// sorted values vs (ascending, no NaN) and their source positions idx: rank[idx[p]] = the average 1-based rank of p's tie run
__global__ __launch_bounds__(RB) void sim_rank_kernel(int64_t N, const double *__restrict__ vs, const int64_t *__restrict__ idx,
                                                      double *__restrict__ rank)
{
    for (int64_t p = (int64_t)blockIdx.x * RB + threadIdx.x; p < N; p += (int64_t)gridDim.x * RB) {
        const double v = vs[p];
        int64_t lo = 0, hi = p;              // first q with !(vs[q] < v)
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (vs[mid] < v) lo = mid + 1; else hi = mid;
        }
        const int64_t first = lo;
        lo = p + 1;
        hi = N;                              // first q with v < vs[q]
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (v < vs[mid]) hi = mid; else lo = mid + 1;
        }
        const int64_t q = idx[p];
        if (q >= 0 && q < N) rank[q] = (double)(first + 1 + lo) * 0.5;
    }
}

// part[b*3 + {0, 1, 2}] = block b's Σ (rx-μ)(ry-μ), Σ (rx-μ)², Σ (ry-μ)²
__global__ __launch_bounds__(RB) void sim_corr_kernel(int64_t N, const double *__restrict__ rx, const double *__restrict__ ry, double mu,
                                                      double *__restrict__ part)
{
    __shared__ double sh[RB];
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * RB + threadIdx.x; k < N; k += (int64_t)gridDim.x * RB) {
        const double dx = rx[k] - mu, dy = ry[k] - mu;
        sxy = sxy + dx * dy;
        sxx = sxx + dx * dx;
        syy = syy + dy * dy;
    }
    sxy = block_sum<RB>(sxy, sh);
    sxx = block_sum<RB>(sxx, sh);
    syy = block_sum<RB>(syy, sh);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = sxy;
        part[3 * blockIdx.x + 1] = sxx;
        part[3 * blockIdx.x + 2] = syy;
    }
}

}  // namespace

static inline unsigned blocks_of(int64_t work, int per) { return (unsigned)((work + per - 1) / per); }

extern "C" int64_t ctgcn_sim_panel_cols(int64_t m, int64_t nnz)
{
    if (m < 1) return 0;
    const int64_t a_bytes = nnz * 12 + (m + 1) * 4;
    const int64_t budget = (int64_t)CACHE_BUDGET - a_bytes;
    int64_t p = budget > 0 ? budget / (2 * 8 * m) : 1;
    if (p >= 64) p &= ~(int64_t)63;
    if (p < 1) p = 1;
    return p < m ? p : m;
}

extern "C" size_t ctgcn_sim_series_workspace_bytes(int64_t m, int64_t panel)
{
    if (m < 1 || panel < 1) return 0;
    if (panel > m) panel = m;
    return (size_t)2 * sizeof(double) * (size_t)m * (size_t)panel;
}

extern "C" int ctgcn_sim_series(int64_t m, const int32_t *row_ptr, const int32_t *col, const double *val, double c, int32_t iter_num,
                                int64_t panel, int64_t col0, int64_t col1, double *S, void *workspace, size_t workspace_bytes, void *stream)
{
    if (m < 1 || iter_num < 1 || panel < 1 || col0 < 0 || col1 < col0 || col1 > m)
        return ctgcn_set_error_(CTGCN_E_INVALID, "sim_series: bad sizes (need m >= 1, iter_num >= 1, panel >= 1, 0 <= col0 <= col1 <= m)");
    if (m > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "sim_series: m over 2^31 - 1");
    if (!row_ptr || !col || !val || !S) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_series: null pointer");
    if (panel > m) panel = m;
    if (!workspace || workspace_bytes < ctgcn_sim_series_workspace_bytes(m, panel))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "sim_series: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *X = (double *)workspace, *Y = X + m * panel;
    for (int64_t j0 = col0; j0 < col1; j0 += panel) {
        const int64_t w = col1 - j0 < panel ? col1 - j0 : panel;
        const unsigned g = blocks_of(m * w, ST);
        if (iter_num == 1) {            // S_1 = c·A·0 + I = I
            hipLaunchKernelGGL(sim_eye_kernel, dim3(g), dim3(ST), 0, st, m, w, j0, S + j0, m);
            continue;
        }
        hipLaunchKernelGGL(sim_eye_kernel, dim3(g), dim3(ST), 0, st, m, w, j0, X, w);
        double *src = X, *dst = Y;
        for (int s = 2; s <= iter_num; ++s) {
            const bool last = s == iter_num;
            hipLaunchKernelGGL(sim_step_kernel, dim3(g), dim3(ST), 0, st, m, w, j0, row_ptr, col, val, c, (const double *)src,
                               last ? S + j0 : dst, last ? m : w);
            double *t = src;
            src = dst;
            dst = t;
        }
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_sim_finish_workspace_bytes(int64_t m)
{
    if (m < 1) return 0;
    const size_t T = (size_t)((m + TT - 1) / TT);
    return sizeof(double) * 2 * T * T;
}

extern "C" int ctgcn_sim_finish(int64_t m, int32_t pad_zero, double eps, double *S, double *stats_out, int64_t *row_nnz, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    if (m < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_finish: m < 1");
    if (m > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "sim_finish: m over 2^31 - 1");
    if (!S || !stats_out || !row_nnz) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_finish: null pointer");
    if (!workspace || workspace_bytes < ctgcn_sim_finish_workspace_bytes(m))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "sim_finish: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t T = (m + TT - 1) / TT;
    if (T > 65535) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "sim_finish: m over 65535 tiles of 32");
    double *part = (double *)workspace;
    hipLaunchKernelGGL(sim_sym_kernel, dim3((unsigned)T, (unsigned)T), dim3(ST), 0, st, m, T, S, part);
    hipLaunchKernelGGL(sim_minmax_reduce_kernel, dim3(1), dim3(RB), 0, st, T * T, (const double *)part, (int)(pad_zero != 0), stats_out);
    hipLaunchKernelGGL(sim_norm_kernel, dim3((unsigned)m), dim3(ST), 0, st, m, S, (const double *)stats_out, eps, row_nnz);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_sim_coo(int64_t m, const double *S, const int64_t *row_off, const int64_t *ids, int32_t *row_out, int32_t *col_out,
                             double *data_out, void *stream)
{
    if (m < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_coo: m < 1");
    if (m > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "sim_coo: m over 2^31 - 1");
    if (!S || !row_off || !ids || !row_out || !col_out || !data_out) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_coo: null pointer");
    hipLaunchKernelGGL(sim_coo_kernel, dim3((unsigned)m), dim3(ST), 0, (hipStream_t)stream, m, S, row_off, ids, row_out, col_out, data_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

template <typename T>
static int sim_gram(const char *name, int64_t m, int32_t d, const T *E, int64_t lde, const int64_t *rows, double *out, void *stream)
{
    char buf[160];
    if (m < 1 || d < 1 || lde < d) {
        snprintf(buf, sizeof(buf), "%s: bad sizes (need m >= 1, d >= 1, lde >= d)", name);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    if (!E || !rows || !out) {
        snprintf(buf, sizeof(buf), "%s: null pointer", name);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    const int64_t Tn = (m + TT - 1) / TT;
    if (Tn > 65535) {
        snprintf(buf, sizeof(buf), "%s: m over 65535 tiles of 32", name);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    hipLaunchKernelGGL(sim_gram_kernel<T>, dim3((unsigned)Tn, (unsigned)Tn), dim3(ST), 0, (hipStream_t)stream, m, (int)d, E, lde, rows, out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_sim_gram_f32(int64_t m, int32_t d, const float *E, int64_t lde, const int64_t *rows, double *out, void *stream)
{
    return sim_gram("sim_gram_f32", m, d, E, lde, rows, out, stream);
}

extern "C" int ctgcn_sim_gram_f64(int64_t m, int32_t d, const double *E, int64_t lde, const int64_t *rows, double *out, void *stream)
{
    return sim_gram("sim_gram_f64", m, d, E, lde, rows, out, stream);
}

extern "C" size_t ctgcn_sim_normalize_workspace_bytes(int64_t N)
{
    if (N < 1) return 0;
    const size_t chunks = (size_t)((N + NP_BUF - 1) / NP_BUF), mm = 2 * (size_t)red_blocks(N);
    return sizeof(double) * (chunks > mm ? chunks : mm);
}

extern "C" int ctgcn_sim_normalize(int64_t N, double *x, double *stats_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_normalize: N < 1");
    if (!x || !stats_out) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_normalize: null pointer");
    if (!workspace || workspace_bytes < ctgcn_sim_normalize_workspace_bytes(N))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "sim_normalize: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t G = red_blocks(N);
    double *part = (double *)workspace;
    hipLaunchKernelGGL(sim_minmax_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, (const double *)x, part);
    hipLaunchKernelGGL(sim_minmax_reduce_kernel, dim3(1), dim3(RB), 0, st, G, (const double *)part, 0, stats_out);
    hipLaunchKernelGGL(sim_scale_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, x, (const double *)stats_out);
    const int64_t chunks = (N + NP_BUF - 1) / NP_BUF;
    hipLaunchKernelGGL(sim_np_chunk_kernel, dim3(blocks_of(chunks, RB)), dim3(RB), 0, st, N, (const double *)x, part);
    hipLaunchKernelGGL(sim_np_total_kernel, dim3(1), dim3(64), 0, st, chunks, (const double *)part, stats_out + 2);
    hipLaunchKernelGGL(sim_div_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, x, (const double *)stats_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_sim_spearman_workspace_bytes(int64_t N)
{
    if (N < 1) return 0;
    return sizeof(double) * (2 * (size_t)N + 3 * (size_t)red_blocks(N));
}

extern "C" int ctgcn_sim_spearman(int64_t N, const double *xs, const int64_t *xi, const double *ys, const int64_t *yi, double *sums_out,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_spearman: N < 1");
    if (!xs || !xi || !ys || !yi || !sums_out) return ctgcn_set_error_(CTGCN_E_INVALID, "sim_spearman: null pointer");
    if (!workspace || workspace_bytes < ctgcn_sim_spearman_workspace_bytes(N))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "sim_spearman: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t G = red_blocks(N);
    double *rx = (double *)workspace, *ry = rx + N, *part = ry + N;
    hipLaunchKernelGGL(sim_rank_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, xs, xi, rx);
    hipLaunchKernelGGL(sim_rank_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, ys, yi, ry);
    hipLaunchKernelGGL(sim_corr_kernel, dim3((unsigned)G), dim3(RB), 0, st, N, (const double *)rx, (const double *)ry,
                       ((double)N + 1.0) * 0.5, part);
    hipLaunchKernelGGL(sim_sum_reduce_kernel, dim3(1), dim3(RB), 0, st, G, 3, (const double *)part, sums_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
