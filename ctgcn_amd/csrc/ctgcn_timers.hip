// ctgcn_timers.hip — the fp64 linear algebra of the TIMERS baseline (reference baseline/timers.py): the passes behind a truncated
// eigendecomposition of a CSR operator (ops.sym_topk), the edge-gather loss, the TRIP update and the matrix-free restart bound.
//
//   - spmm_f64_kernel: Y = A·X or Y += A·X on [n, b] blocks.  A group of LPR lanes owns a row and walks its entries in CSR order, each
//     lane with up to four columns (l, l + LPR, l + 2 LPR, l + 3 LPR) in registers, so an entry costs one coalesced gather per column
//     slice and an empty row or a row of thousands of entries is the same loop.  LPR is the smallest power of two with 4 LPR >= b, at
//     most 64; past 256 columns the row is walked once per 256.  The long-row pieces of ctgcn_gather.h are not used: that scaffold is
//     float4 and takes the caller's long-row list and workspace, and the blocks here are 40 to 136 doubles wide, where a single
//     group already has a row's whole width in flight.
//   - tsgemm_tn_kernel: G = XᵀY over n rows, 64 x 64 output tiles, the rows cut into P runs (tn_parts) with one partial per run,
//     summed in run order by part_sum_kernel; P = 1 writes G directly.
//   - tsgemm_nn_kernel: Y = X·C, 64 rows x 64 columns a block, with the block's column sums of squares of Y as an optional partial
//     (TRIP's normalisation, the solver's residual norms), summed in block order.
//   - timers_obj_kernel: Σ s² (or Σ (s_old + s − ⟨U_r, V_c⟩)² − (s_old − ⟨U_r, V_c⟩)²) and Σ s ⟨U_r, V_c⟩ over the stored entries; LPR
//     lanes take a row, split the length-k dot and close it with a fixed xor tree; block partials, then one block.
//
// Arithmetic: plain v_fma_f64 on 4 x 4 register tiles fed from LDS, not v_mfma_f64_16x16x4_f64.  On gfx950 the fp64 vector and matrix
// peaks are equal, the products here stream n·b doubles against b² (or nnz·b) flops and sit on memory, and the fp64 MFMA's C/D
// layout differs from every other MFMA's, so the matrix path would buy no rate for a second layout to keep right.  Neither has been
// timed against the other.
// No float atomics: every reduction is per-block partials summed in a fixed order, and the partial counts depend on the sizes alone,
// so repeated calls are bit-identical (the restart decision is a comparison of two such sums).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "ctgcn_reduce.h"
#include "ctgcn_try.h"

namespace {

constexpr int TB = 256;                   // every block here
constexpr int TS_MAXB = 512;              // widest block of the tall-skinny products (tsgemm_nn's X: two blocks side by side)
constexpr int TILE = 64;                  // output tile edge of both products: 4 x 4 a thread
constexpr int KS = 16;                    // depth of one LDS stage
constexpr int64_t TN_ROWS = 512;          // fewest rows of a run of tsgemm_tn
constexpr int TN_MAX_PART = 1024;         // output tiles x runs stays below this
constexpr int OBJ_MAX_BLOCKS = 1024;

__host__ __device__ __forceinline__ int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------- SpMM

template <int LPR>
__global__ __launch_bounds__(TB) void spmm_f64_kernel(int64_t n, int b, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ X, int64_t ldx,
                                                      double *__restrict__ Y, int64_t ldy, int accumulate)
{
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int64_t i = (int64_t)blockIdx.x * (TB / LPR) + g;
    if (i >= n) return;
    const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
    for (int c0 = 0; c0 < b; c0 += 4 * LPR) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        bool on[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) on[j] = c0 + l + j * LPR < b;
#pragma unroll 2
        for (int e = e0; e < e1; ++e) {
            const double a = val[e];
            const double *x = X + (int64_t)col[e] * ldx + c0 + l;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (on[j]) acc[j] = fma(a, x[j * LPR], acc[j]);
        }
        double *y = Y + i * ldy + c0 + l;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (on[j]) y[j * LPR] = accumulate ? y[j * LPR] + acc[j] : acc[j];
    }
}

// ---------------------------------------------------------------- tall-skinny products

// runs of tsgemm_tn over n rows: from the sizes alone
int64_t tn_parts(int64_t n, int b1, int b2)
{
    const int64_t tiles = cdiv(b1, TILE) * cdiv(b2, TILE);
    const int64_t cap = TN_MAX_PART / tiles < 1 ? 1 : TN_MAX_PART / tiles;
    int64_t P = cdiv(n, TN_ROWS);
    P = P < 1 ? 1 : (P > cap ? cap : P);
    return cdiv(n, cdiv(n, P));           // no empty run
}

// block (tile, run): part[run][b1][b2] tile = Σ over the run's rows of X[r, i]·Y[r, j], rows in order
__global__ __launch_bounds__(TB) void tsgemm_tn_kernel(int64_t n, int b1, int b2, const double *__restrict__ X, int64_t ldx,
                                                       const double *__restrict__ Y, int64_t ldy, int64_t rows_per, double *__restrict__ part)
{
    __shared__ double Xs[KS][TILE], Ys[KS][TILE];
    const int tiles2 = (b2 + TILE - 1) / TILE;
    const int i0 = (blockIdx.x / tiles2) * TILE, j0 = (blockIdx.x % tiles2) * TILE;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16, lc = threadIdx.x % TILE, lr = threadIdx.x / TILE;
    double acc[4][4] = {};
    for (int64_t r = r0; r < r1; r += KS) {
#pragma unroll
        for (int q = 0; q < KS / 4; ++q) {
            const int rr = lr + 4 * q;
            const int64_t row = r + rr;
            Xs[rr][lc] = (row < r1 && i0 + lc < b1) ? X[row * ldx + i0 + lc] : 0.0;
            Ys[rr][lc] = (row < r1 && j0 + lc < b2) ? Y[row * ldy + j0 + lc] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            double a[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = Xs[k][ty * 4 + u];
                c[u] = Ys[k][tx * 4 + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], c[v], acc[u][v]);
        }
        __syncthreads();
    }
    double *out = part + (int64_t)blockIdx.y * b1 * b2;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < b1 && j < b2) out[(int64_t)i * b2 + j] = acc[u][v];
        }
}

// out[i] = Σ_p part[p*per + i], p in order
__global__ __launch_bounds__(TB) void part_sum_kernel(int64_t P, int64_t per, const double *__restrict__ part, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= per) return;
    double s = 0.0;
    for (int64_t p = 0; p < P; ++p) s += part[p * per + i];
    out[i] = s;
}

// block (row tile, column tile): Y tile = X[rows, :]·C[:, columns]; part[row tile][b2] = the tile's column sums of Y² (part null: none)
__global__ __launch_bounds__(TB) void tsgemm_nn_kernel(int64_t n, int b1, int b2, const double *__restrict__ X, int64_t ldx,
                                                       const double *__restrict__ C, int64_t ldc, double *__restrict__ Y, int64_t ldy,
                                                       double *__restrict__ part)
{
    __shared__ double Xs[KS][TILE + 1], Cs[KS][TILE], sq[16][TILE];
    const int64_t r0 = (int64_t)blockIdx.x * TILE;
    const int c0 = blockIdx.y * TILE;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16, lc = threadIdx.x % TILE, lr = threadIdx.x / TILE;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < b1; k0 += KS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rr = ty + 16 * q;            // X: 64 rows x 16 deep, the depth across 16 lanes
            Xs[tx][rr] = (r0 + rr < n && k0 + tx < b1) ? X[(r0 + rr) * ldx + k0 + tx] : 0.0;
            const int kk = lr + 4 * q;             // C: 16 deep x 64 columns
            Cs[kk][lc] = (k0 + kk < b1 && c0 + lc < b2) ? C[(int64_t)(k0 + kk) * ldc + c0 + lc] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            double a[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = Xs[k][ty * 4 + u];
                c[u] = Cs[k][tx * 4 + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], c[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t i = r0 + ty * 4 + u;
            const int j = c0 + tx * 4 + v;
            if (i < n && j < b2) Y[i * ldy + j] = acc[u][v];
        }
    if (!part) return;                            // (uniform)
#pragma unroll
    for (int v = 0; v < 4; ++v) {                  // rows past n hold zeros
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s = fma(acc[u][v], acc[u][v], s);
        sq[ty][tx * 4 + v] = s;
    }
    __syncthreads();
    if (threadIdx.x < TILE && c0 + (int)threadIdx.x < b2) {
        double s = 0.0;
#pragma unroll
        for (int y = 0; y < 16; ++y) s += sq[y][threadIdx.x];
        part[(int64_t)blockIdx.x * b2 + c0 + threadIdx.x] = s;
    }
}

// ---------------------------------------------------------------- the edge-gather loss

int obj_lanes(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

int64_t obj_blocks(int64_t n, int k)
{
    const int64_t groups = TB / obj_lanes(k);
    int64_t NB = cdiv(n, groups * 4);
    NB = NB < 1 ? 1 : (NB > OBJ_MAX_BLOCKS ? OBJ_MAX_BLOCKS : NB);
    return cdiv(n, cdiv(n, NB));
}

// part[2 blk] = Σ s² (s_old: Σ (s_old + s − d)² − (s_old − d)²), part[2 blk + 1] = Σ s·d, d = ⟨U_row, V_col⟩, over the block's rows
template <int LPR>
__global__ __launch_bounds__(TB) void timers_obj_kernel(int64_t n, int k, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const double *__restrict__ s, const double *__restrict__ s_old,
                                                        const double *__restrict__ U, int64_t ldu, const double *__restrict__ V, int64_t ldv,
                                                        int64_t rows_per, double *__restrict__ part)
{
    __shared__ double sh[TB];
    const int g = threadIdx.x / LPR, l = threadIdx.x % LPR;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = r0 + g; i < r1; i += TB / LPR) {
        const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
        const double *u = U + i * ldu;
        for (int e = e0; e < e1; ++e) {
            const double *v = V + (int64_t)col[e] * ldv;
            double d = 0.0;
            for (int j = l; j < k; j += LPR) d = fma(u[j], v[j], d);
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, LPR);
            if (l == 0) {
                const double sv = s[e];
                a1 = fma(sv, d, a1);
                if (s_old) {
                    const double so = s_old[e], p = so + sv - d, q = so - d;
                    a0 += p * p - q * q;
                } else {
                    a0 = fma(sv, sv, a0);
                }
            }
        }
    }
    a0 = block_sum<TB>(a0, sh);
    a1 = block_sum<TB>(a1, sh);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = a0;
        part[2 * (int64_t)blockIdx.x + 1] = a1;
    }
}

__global__ __launch_bounds__(TB) void timers_obj_final_kernel(int64_t NB, const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double sh[TB];
    double a0 = 0.0, a1 = 0.0;
    for (int64_t b = threadIdx.x; b < NB; b += TB) {
        a0 += part[2 * b];
        a1 += part[2 * b + 1];
    }
    a0 = block_sum<TB>(a0, sh);
    a1 = block_sum<TB>(a1, sh);
    if (threadIdx.x == 0) {
        out[0] = a0;
        out[1] = a1;
    }
}

template <int LPR>
void launch_spmm(hipStream_t st, int64_t n, int b, const int32_t *row_ptr, const int32_t *col, const double *val, const double *X, int64_t ldx,
                 double *Y, int64_t ldy, int accumulate)
{
    hipLaunchKernelGGL(spmm_f64_kernel<LPR>, dim3((unsigned)cdiv(n, TB / LPR)), dim3(TB), 0, st, n, b, row_ptr, col, val, X, ldx, Y, ldy,
                       accumulate);
}

template <int LPR>
void launch_obj(hipStream_t st, int64_t NB, int64_t n, int k, const int32_t *row_ptr, const int32_t *col, const double *s, const double *s_old,
                const double *U, int64_t ldu, const double *V, int64_t ldv, double *part)
{
    hipLaunchKernelGGL(timers_obj_kernel<LPR>, dim3((unsigned)NB), dim3(TB), 0, st, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, cdiv(n, NB),
                       part);
}

int bad_ts(const char *what, int64_t n, int32_t b1, int32_t b2, int32_t max_b1)
{
    if (n < 0 || b1 < 1 || b2 < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "bad sizes (need n >= 0, b1 >= 1, b2 >= 1)");
    if (b1 > max_b1 || b2 > TS_MAXB) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "a block wider than the limit (ctgcn_hip.h)");
    return CTGCN_OK;
}

}  // namespace

extern "C" int ctgcn_spmm_csr_f64(int64_t n_rows, int32_t b, const int32_t *row_ptr, const int32_t *col_idx, const double *val, const double *X,
                                  int64_t ldx, double *Y, int64_t ldy, int accumulate, void *stream)
{
    if (n_rows < 0 || n_rows > INT32_MAX || b < 1 || ldx < b || ldy < b)
        return ctgcn_fail(CTGCN_E_INVALID, "spmm_csr_f64", "bad sizes (need 0 <= n < 2^31, b >= 1, ldx >= b, ldy >= b)");
    if (n_rows == 0) return CTGCN_OK;
    if (!row_ptr || !col_idx || !val || !X || !Y) return ctgcn_fail(CTGCN_E_INVALID, "spmm_csr_f64", "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int lpr = b <= 4 ? 1 : b <= 8 ? 2 : b <= 16 ? 4 : b <= 32 ? 8 : b <= 64 ? 16 : b <= 128 ? 32 : 64;
    switch (lpr) {
    case 1: launch_spmm<1>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    case 2: launch_spmm<2>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    case 4: launch_spmm<4>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    case 8: launch_spmm<8>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    case 16: launch_spmm<16>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    case 32: launch_spmm<32>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    default: launch_spmm<64>(st, n_rows, b, row_ptr, col_idx, val, X, ldx, Y, ldy, accumulate); break;
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_tsgemm_tn_workspace_bytes(int64_t n, int32_t b1, int32_t b2)
{
    if (n < 1 || b1 < 1 || b2 < 1 || b1 > TS_MAXB || b2 > TS_MAXB) return 0;
    const int64_t P = tn_parts(n, b1, b2);
    return P > 1 ? sizeof(double) * (size_t)P * b1 * b2 : 0;
}

extern "C" int ctgcn_tsgemm_tn_f64(int64_t n, int32_t b1, int32_t b2, const double *X, int64_t ldx, const double *Y, int64_t ldy, double *G,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = bad_ts("tsgemm_tn_f64", n, b1, b2, TS_MAXB)) return rc;
    if (ldx < b1 || ldy < b2) return ctgcn_fail(CTGCN_E_INVALID, "tsgemm_tn_f64", "a leading dimension below its width");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (G) CTGCN_TRY(hipMemsetAsync(G, 0, sizeof(double) * (size_t)b1 * b2, st));
        return CTGCN_OK;
    }
    if (!X || !Y || !G) return ctgcn_fail(CTGCN_E_INVALID, "tsgemm_tn_f64", "null pointer");
    const int64_t P = tn_parts(n, b1, b2);
    if (P > 1 && (!workspace || workspace_bytes < ctgcn_tsgemm_tn_workspace_bytes(n, b1, b2)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, "tsgemm_tn_f64", "workspace too small");
    const unsigned tiles = (unsigned)(cdiv(b1, TILE) * cdiv(b2, TILE));
    double *part = P > 1 ? (double *)workspace : G;
    hipLaunchKernelGGL(tsgemm_tn_kernel, dim3(tiles, (unsigned)P), dim3(TB), 0, st, n, (int)b1, (int)b2, X, ldx, Y, ldy, cdiv(n, P), part);
    if (P > 1) {
        const int64_t per = (int64_t)b1 * b2;
        hipLaunchKernelGGL(part_sum_kernel, dim3((unsigned)cdiv(per, TB)), dim3(TB), 0, st, P, per, (const double *)part, G);
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_tsgemm_nn_workspace_bytes(int64_t n, int32_t b2)
{
    if (n < 1 || b2 < 1 || b2 > TS_MAXB) return 0;
    return sizeof(double) * (size_t)cdiv(n, TILE) * b2;
}

extern "C" int ctgcn_tsgemm_nn_f64(int64_t n, int32_t b1, int32_t b2, const double *X, int64_t ldx, const double *C, int64_t ldc, double *Y,
                                   int64_t ldy, double *colsq, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = bad_ts("tsgemm_nn_f64", n, b1, b2, 2 * TS_MAXB)) return rc;
    if (ldx < b1 || ldc < b2 || ldy < b2) return ctgcn_fail(CTGCN_E_INVALID, "tsgemm_nn_f64", "a leading dimension below its width");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (colsq) CTGCN_TRY(hipMemsetAsync(colsq, 0, sizeof(double) * (size_t)b2, st));
        return CTGCN_OK;
    }
    if (!X || !C || !Y) return ctgcn_fail(CTGCN_E_INVALID, "tsgemm_nn_f64", "null pointer");
    if (colsq && (!workspace || workspace_bytes < ctgcn_tsgemm_nn_workspace_bytes(n, b2)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, "tsgemm_nn_f64", "workspace too small");
    const int64_t RT = cdiv(n, TILE);
    double *part = colsq ? (double *)workspace : nullptr;
    hipLaunchKernelGGL(tsgemm_nn_kernel, dim3((unsigned)RT, (unsigned)cdiv(b2, TILE)), dim3(TB), 0, st, n, (int)b1, (int)b2, X, ldx, C, ldc, Y, ldy,
                       part);
    if (colsq) hipLaunchKernelGGL(part_sum_kernel, dim3((unsigned)cdiv(b2, TB)), dim3(TB), 0, st, RT, (int64_t)b2, (const double *)part, colsq);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_timers_obj_workspace_bytes(int64_t n, int32_t k)
{
    if (n < 1 || k < 1) return 0;
    return sizeof(double) * 2 * (size_t)obj_blocks(n, k);
}

extern "C" int ctgcn_timers_obj_f64(int64_t n, int32_t k, const int32_t *row_ptr, const int32_t *col, const double *s, const double *s_old,
                                    const double *U, int64_t ldu, const double *V, int64_t ldv, double *out, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > INT32_MAX || k < 1 || ldu < k || ldv < k)
        return ctgcn_fail(CTGCN_E_INVALID, "timers_obj_f64", "bad sizes (need 0 <= n < 2^31, k >= 1, ldu >= k, ldv >= k)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (out) CTGCN_TRY(hipMemsetAsync(out, 0, sizeof(double) * 2, st));
        return CTGCN_OK;
    }
    if (!row_ptr || !col || !s || !U || !V || !out) return ctgcn_fail(CTGCN_E_INVALID, "timers_obj_f64", "null pointer");
    if (!workspace || workspace_bytes < ctgcn_timers_obj_workspace_bytes(n, k))
        return ctgcn_fail(CTGCN_E_WORKSPACE, "timers_obj_f64", "workspace too small");
    const int64_t NB = obj_blocks(n, k);
    double *part = (double *)workspace;
    switch (obj_lanes(k)) {
    case 1: launch_obj<1>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    case 2: launch_obj<2>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    case 4: launch_obj<4>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    case 8: launch_obj<8>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    case 16: launch_obj<16>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    case 32: launch_obj<32>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    default: launch_obj<64>(st, NB, n, k, row_ptr, col, s, s_old, U, ldu, V, ldv, part); break;
    }
    hipLaunchKernelGGL(timers_obj_final_kernel, dim3(1), dim3(TB), 0, st, NB, (const double *)part, out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
