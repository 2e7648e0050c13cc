// ctgcn_cent.hip — centrality-prediction evaluation (reference evaluation/centrality_prediction.py) on the GPU.
//
//   - brandes_kernel: exact Brandes betweenness and the closeness counts (r, D) of a source range, one level-synchronous BFS per
//     source.  A persistent grid: block b owns sources s0 + b, s0 + b + G, ... and a private state slab in global memory (dist,
//     sigma, delta, the BFS-ordered vertex list, level offsets and its betweenness partial).  Discovery pushes with an atomicCAS on
//     dist; sigma (path counts) and delta (dependencies) are then PULLED over each vertex's CSR row in CSR order, so they do not
//     depend on the order in which vertices were discovered.  A group of W lanes (W from the level's size, 4..64) shares one vertex
//     and its row; its lane partials are summed by a fixed butterfly.
//   - eig_*_kernel: the networkx power iteration x <- (A + I) x / ||(A + I) x||, all max_iter steps enqueued at once; a device flag
//     set by the stop test turns the later steps into no-ops, and one read at the end returns the stop step.
//   - ridge_gram_kernel / ridge_sse_kernel: the two passes of the k-fold ridge regression: per-fold augmented Grams [X 1]ᵀ[X 1 Y]
//     and the held-out squared errors of every (alpha, target) model.
// No float atomics anywhere: per-block partials are summed in a fixed order, so repeated calls are bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "ctgcn_reduce.h"
#include "ctgcn_try.h"

namespace {

constexpr int BT = 256;                          // Brandes block
constexpr int MAX_BR_BLOCKS = 512;               // persistent grid cap: 2 blocks per CU
constexpr size_t BR_BUDGET = (size_t)2 << 30;    // state slabs of all blocks
constexpr int RT = 256;                          // reduction / eigenvector / ridge blocks
constexpr int MAX_EIG_BLOCKS = 1024;
constexpr int RIDGE_MAXD = 512;
constexpr int RIDGE_MAXT = 8;
constexpr int RIDGE_MAXP = 64;
constexpr int RIDGE_CHUNKS = 16;                 // row chunks per fold (partials summed in chunk order)
constexpr int GT = 64;                           // Gram output tile (GT x GT per block)
constexpr int GK = 32;                           // rows per LDS stage of the Gram pass
constexpr int SSE_SPLIT = 8;                     // blocks per row chunk of the squared-error pass

// dist is written by atomicCAS (performed in L2) and read by other waves: read it at agent scope so a stale L1 line is never used
__device__ __forceinline__ int ld_dist(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Barrier of the Brandes block.  The fence first: plain stores (the dist reset, sigma, delta) must be complete in L2 before another
// wave's atomicCAS or agent-scope load can race them, and it drops the CU's L1 lines written under it
__device__ __forceinline__ void bar()
{
    __threadfence();
    __syncthreads();
}

__device__ __forceinline__ int group_width(int count)
{
    if (count <= BT / 64) return 64;
    int w = 64;
    while (w > 4 && w * count > BT) w >>= 1;
    return w;
}

__device__ __forceinline__ double group_sum(double v, int W)
{
    for (int m = W >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, W);
    return v;
}

size_t slab_bytes(int64_t n) { return (((size_t)3 * 8 * n + (size_t)4 * (3 * n + 2)) + 255) & ~(size_t)255; }

int brandes_blocks(int64_t n, int64_t nsrc)
{
    const int64_t by_mem = std::max<int64_t>(1, (int64_t)(BR_BUDGET / slab_bytes(n)));
    return (int)std::max<int64_t>(1, std::min<int64_t>({nsrc, (int64_t)MAX_BR_BLOCKS, by_mem}));
}

__global__ __launch_bounds__(BT) void brandes_kernel(int n, const int *__restrict__ rp, const int *__restrict__ col, int s0, int s1,
                                                    char *__restrict__ ws, size_t slab, int64_t *__restrict__ r_out,
                                                    int64_t *__restrict__ D_out)
{
    char *base = ws + (size_t)blockIdx.x * slab;
    double *sigma = (double *)base;
    double *delta = sigma + n;
    double *bcp = delta + n;
    int *dist = (int *)(bcp + n);
    int *queue = dist + n;
    int *lvl = queue + n;               // lvl[k] = start of level k in queue
    __shared__ int s_tail;
    const int tid = threadIdx.x;
    for (int v = tid; v < n; v += BT) {
        dist[v] = -1;
        bcp[v] = 0.0;
    }
    bar();
    for (int s = s0 + (int)blockIdx.x; s < s1; s += (int)gridDim.x) {
        if (rp[s + 1] == rp[s]) {       // no neighbours: r = 1, D = 0, no dependencies
            if (tid == 0) {
                r_out[s - s0] = 1;
                D_out[s - s0] = 0;
            }
            continue;
        }
        if (tid == 0) {
            dist[s] = 0;
            sigma[s] = 1.0;
            queue[0] = s;
            lvl[0] = 0;
            lvl[1] = 1;
            s_tail = 1;
        }
        bar();
        int L = 0, lo = 0, hi = 1;
        int64_t D = 0;
        for (;;) {
            {   // discover level L + 1 from the frontier queue[lo, hi)
                const int W = group_width(hi - lo), g = tid / W, lane = tid % W, ng = BT / W;
                for (int i = lo + g; i < hi; i += ng) {
                    const int v = queue[i];
                    for (int e = rp[v] + lane; e < rp[v + 1]; e += W) {
                        const int w = col[e];
                        if (ld_dist(dist + w) < 0 && atomicCAS(dist + w, -1, L + 1) == -1) queue[atomicAdd(&s_tail, 1)] = w;
                    }
                }
            }
            bar();
            const int nhi = s_tail;
            if (nhi == hi) break;
            {   // sigma of the new level: pull over each row, in CSR order
                const int W = group_width(nhi - hi), g = tid / W, lane = tid % W, ng = BT / W;
                for (int i = hi + g; i < nhi; i += ng) {
                    const int w = queue[i];
                    double acc = 0.0;
                    for (int e = rp[w] + lane; e < rp[w + 1]; e += W) {
                        const int v = col[e];
                        if (ld_dist(dist + v) == L) acc += sigma[v];
                    }
                    acc = group_sum(acc, W);
                    if (lane == 0) sigma[w] = acc;
                }
            }
            if (tid == 0) lvl[L + 2] = nhi;
            D += (int64_t)(L + 1) * (nhi - hi);
            bar();
            lo = hi;
            hi = nhi;
            ++L;
        }
        // levels 0..L; backward sweep from the deepest level: delta[v] = sigma[v] Σ_{w succ v} (1 + delta[w]) / sigma[w]
        for (int k = L; k >= 1; --k) {
            const int a = lvl[k], b = lvl[k + 1];
            const int W = group_width(b - a), g = tid / W, lane = tid % W, ng = BT / W;
            for (int i = a + g; i < b; i += ng) {
                const int v = queue[i];
                double acc = 0.0;
                for (int e = rp[v] + lane; e < rp[v + 1]; e += W) {
                    const int w = col[e];
                    if (ld_dist(dist + w) == k + 1) acc += (1.0 + delta[w]) / sigma[w];
                }
                acc = group_sum(acc, W);
                if (lane == 0) {
                    const double dv = sigma[v] * acc;
                    delta[v] = dv;
                    bcp[v] += dv;
                }
            }
            bar();
        }
        for (int i = tid; i < hi; i += BT) dist[queue[i]] = -1;
        if (tid == 0) {
            r_out[s - s0] = hi;
            D_out[s - s0] = D;
        }
        bar();
    }
}

// out[v] = Σ_b part[b * stride + v], b in order
__global__ __launch_bounds__(RT) void slab_reduce_kernel(int64_t n, int blocks, int64_t stride, const double *__restrict__ part,
                                                         double *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (v >= n) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(int64_t)b * stride + v];
    out[v] = s;
}

struct EigCtrl {
    int done;
    int stop_step;
    double norm;
};

__global__ __launch_bounds__(RT) void eig_init_kernel(int64_t n, double *__restrict__ x, EigCtrl *ctrl)
{
    const int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x;
    if (v < n) x[v] = 1.0 / (double)n;
    if (v == 0) {
        ctrl->done = 0;
        ctrl->stop_step = 0;
        ctrl->norm = 1.0;
    }
}

// y = x + A x by rows; part[b] = Σ y² over this block's rows
__global__ __launch_bounds__(RT) void eig_spmv_kernel(int64_t n, const int *__restrict__ rp, const int *__restrict__ col,
                                                      const double *__restrict__ x, double *__restrict__ y, double *__restrict__ part,
                                                      const EigCtrl *ctrl)
{
    __shared__ double sh[RT];
    if (ctrl->done) return;
    double sq = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x; v < n; v += (int64_t)gridDim.x * RT) {
        double acc = x[v];
        for (int e = rp[v]; e < rp[v + 1]; ++e) acc += x[col[e]];
        y[v] = acc;
        sq += acc * acc;
    }
    sq = block_sum<RT>(sq, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

__global__ __launch_bounds__(RT) void eig_norm_kernel(int blocks, const double *__restrict__ part, EigCtrl *ctrl)
{
    __shared__ double sh[RT];
    if (ctrl->done) return;
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += RT) s += part[b];
    s = block_sum<RT>(s, sh);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(s);
        ctrl->norm = nrm == 0.0 ? 1.0 : nrm;
    }
}

// x <- y / norm; part[b] = Σ |x_new - x_last| over this block's rows
__global__ __launch_bounds__(RT) void eig_scale_kernel(int64_t n, const double *__restrict__ y, double *__restrict__ x,
                                                       double *__restrict__ part, const EigCtrl *ctrl)
{
    __shared__ double sh[RT];
    if (ctrl->done) return;
    const double nrm = ctrl->norm;
    double ch = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x; v < n; v += (int64_t)gridDim.x * RT) {
        const double xn = y[v] / nrm;
        ch += fabs(xn - x[v]);
        x[v] = xn;
    }
    ch = block_sum<RT>(ch, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = ch;
}

__global__ __launch_bounds__(RT) void eig_test_kernel(int blocks, const double *__restrict__ part, double bound, int step, EigCtrl *ctrl)
{
    __shared__ double sh[RT];
    if (ctrl->done) return;
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += RT) s += part[b];
    s = block_sum<RT>(s, sh);
    if (threadIdx.x == 0 && s < bound) {
        ctrl->done = 1;
        ctrl->stop_step = step;
    }
}

int eig_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + RT - 1) / RT, MAX_EIG_BLOCKS)); }

// KFold(n_splits=F) without shuffling: fold f is rows [start, start + len), the first n % F folds one row longer
__host__ __device__ __forceinline__ void fold_range(int64_t n, int F, int f, int64_t &start, int64_t &len)
{
    const int64_t q = n / F, r = n % F;
    len = q + (f < r ? 1 : 0);
    start = (int64_t)f * q + std::min<int64_t>(f, r);
}

__host__ __device__ __forceinline__ void chunk_range(int64_t n, int F, int f, int c, int64_t &a, int64_t &b)
{
    int64_t start, len;
    fold_range(n, F, f, start, len);
    const int64_t cs = (len + RIDGE_CHUNKS - 1) / RIDGE_CHUNKS;
    a = std::min<int64_t>(start + (int64_t)c * cs, start + len);
    b = std::min<int64_t>(a + cs, start + len);
}

// column j of Z = [X 1 Y] at row r
template <typename TX>
__device__ __forceinline__ double zval(int64_t r, int j, int d, int T, const TX *__restrict__ X, int64_t ldx, const double *__restrict__ Y)
{
    if (j < d) return (double)X[r * ldx + j];
    if (j == d) return 1.0;
    if (j < d + 1 + T) return Y[r * T + (j - d - 1)];
    return 0.0;
}

// part[(f * CHUNKS + c), i, j] = Σ_{rows of chunk c of fold f} Z[r, i] Z[r, j], i < d + 1, j < d + 1 + T
template <typename TX>
__global__ __launch_bounds__(RT) void ridge_gram_kernel(int64_t n, int d, int T, int F, const TX *__restrict__ X, int64_t ldx,
                                                        const double *__restrict__ Y, double *__restrict__ part)
{
    __shared__ double As[GK][GT + 1];
    __shared__ double Bs[GK][GT + 1];
    const int NR = d + 1, NC = d + 1 + T;
    const int tiles_c = (NC + GT - 1) / GT;
    const int i0 = (blockIdx.x / tiles_c) * GT, j0 = (blockIdx.x % tiles_c) * GT;
    const int f = blockIdx.y / RIDGE_CHUNKS, c = blockIdx.y % RIDGE_CHUNKS;
    int64_t a, b;
    chunk_range(n, F, f, c, a, b);
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int64_t r0 = a; r0 < b; r0 += GK) {
        for (int k = threadIdx.x; k < GK * GT; k += RT) {
            const int rr = k / GT, cc = k % GT;
            const int64_t r = r0 + rr;
            const bool in = r < b;
            As[rr][cc] = in && i0 + cc < NR ? zval(r, i0 + cc, d, T, X, ldx, Y) : 0.0;
            Bs[rr][cc] = in && j0 + cc < NC ? zval(r, j0 + cc, d, T, X, ldx, Y) : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < GK; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) av[p] = As[kk][ty + 16 * p];
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[q] = Bs[kk][tx + 16 * q];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(av[p], bv[q], acc[p][q]);
        }
        __syncthreads();
    }
    double *out = part + (size_t)blockIdx.y * NR * NC;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
            if (i < NR && j < NC) out[(size_t)i * NC + j] = acc[p][q];
        }
}

// out[f, e] = Σ_c part[f, c, e], c = 0..chunks-1 in order
__global__ __launch_bounds__(RT) void chunk_reduce_kernel(int64_t per, int chunks, const double *__restrict__ part, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int f = blockIdx.y;
    if (e >= per) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((int64_t)f * chunks + c) * per + e];
    out[(int64_t)f * per + e] = s;
}

// part[((f * CHUNKS + c) * SSE_SPLIT + x), p] = Σ_{rows of chunk c of fold f taken by block x} (Y[r, tgt[p]] - X[r] w_fp - b_fp)², w_fp = W[f, p, :d], b_fp = W[f, p, d].
// One wave per row: lane l holds columns l, l + 64, ...; the dot of every model is a fixed butterfly; lane p keeps model p's sum.
template <typename TX>
__global__ __launch_bounds__(RT) void ridge_sse_kernel(int64_t n, int d, int T, int F, int P, const TX *__restrict__ X, int64_t ldx,
                                                       const double *__restrict__ Y, const double *__restrict__ W,
                                                       const int *__restrict__ tgt, double *__restrict__ part)
{
    __shared__ double sh[RT / 64][RIDGE_MAXP];
    const int f = blockIdx.y / RIDGE_CHUNKS, c = blockIdx.y % RIDGE_CHUNKS;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    int64_t a, b;
    chunk_range(n, F, f, c, a, b);
    const double *Wf = W + (size_t)f * P * (d + 1);
    const int my_t = lane < P ? tgt[lane] : 0;
    const double my_b = lane < P ? Wf[(size_t)lane * (d + 1) + d] : 0.0;
    double acc = 0.0;
    for (int64_t r = a + wave + (int64_t)(RT / 64) * blockIdx.x; r < b; r += (int64_t)(RT / 64) * SSE_SPLIT) {
        double xr[RIDGE_MAXD / 64];
#pragma unroll
        for (int k = 0; k < RIDGE_MAXD / 64; ++k) {
            const int cc = lane + 64 * k;
            xr[k] = cc < d ? (double)X[r * ldx + cc] : 0.0;
        }
        double mine = 0.0;
        for (int p = 0; p < P; ++p) {
            const double *w = Wf + (size_t)p * (d + 1);
            double dot = 0.0;
#pragma unroll
            for (int k = 0; k < RIDGE_MAXD / 64; ++k) {
                const int cc = lane + 64 * k;
                if (cc < d) dot = fma(xr[k], w[cc], dot);
            }
            dot = group_sum(dot, 64);
            if (lane == p) mine = dot;
        }
        if (lane < P) {
            const double res = Y[r * T + my_t] - (mine + my_b);
            acc = fma(res, res, acc);
        }
    }
    if (lane < P) sh[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < P) {
        double s = 0.0;
        for (int w = 0; w < RT / 64; ++w) s += sh[w][threadIdx.x];
        part[((size_t)blockIdx.y * SSE_SPLIT + blockIdx.x) * P + threadIdx.x] = s;
    }
}

}  // namespace

extern "C" size_t ctgcn_cent_brandes_workspace_bytes(int64_t n, int64_t s0, int64_t s1)
{
    if (n < 1 || s0 < 0 || s1 <= s0 || s1 > n) return 0;
    return (size_t)brandes_blocks(n, s1 - s0) * slab_bytes(n);
}

extern "C" int ctgcn_cent_brandes(int64_t n, const int32_t *row_ptr, const int32_t *col, int64_t s0, int64_t s1, double *bc_out,
                                  int64_t *r_out, int64_t *D_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 1 || s0 < 0 || s1 < s0 || s1 > n) return ctgcn_set_error_(CTGCN_E_INVALID, "cent_brandes: bad sizes (need n >= 1, 0 <= s0 <= s1 <= n)");
    if (n > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "cent_brandes: n over 2^31 - 1");
    if (!row_ptr || !col || !bc_out || !r_out || !D_out) return ctgcn_set_error_(CTGCN_E_INVALID, "cent_brandes: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (s1 == s0) {
        CTGCN_TRY(hipMemsetAsync(bc_out, 0, sizeof(double) * n, st));
        return CTGCN_OK;
    }
    if (!workspace || workspace_bytes < ctgcn_cent_brandes_workspace_bytes(n, s0, s1))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "cent_brandes: workspace too small");
    const int G = brandes_blocks(n, s1 - s0);
    const size_t slab = slab_bytes(n);
    hipLaunchKernelGGL(brandes_kernel, dim3(G), dim3(BT), 0, st, (int)n, row_ptr, col, (int)s0, (int)s1, (char *)workspace, slab, r_out, D_out);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((n + RT - 1) / RT)), dim3(RT), 0, st, n, G, (int64_t)(slab / sizeof(double)),
                       (const double *)((char *)workspace + sizeof(double) * 2 * n), bc_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_cent_eigenvector_workspace_bytes(int64_t n)
{
    if (n < 1) return 0;
    return 256 + sizeof(double) * ((size_t)n + eig_blocks(n));
}

extern "C" int ctgcn_cent_eigenvector(int64_t n, const int32_t *row_ptr, const int32_t *col, int32_t max_iter, double tol, double *x_out,
                                      int32_t *stop_step_host, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 1 || max_iter < 0) return ctgcn_set_error_(CTGCN_E_INVALID, "cent_eigenvector: bad sizes (need n >= 1, max_iter >= 0)");
    if (!row_ptr || !col || !x_out || !stop_step_host || !workspace) return ctgcn_set_error_(CTGCN_E_INVALID, "cent_eigenvector: null pointer");
    if (workspace_bytes < ctgcn_cent_eigenvector_workspace_bytes(n))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "cent_eigenvector: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    EigCtrl *ctrl = (EigCtrl *)workspace;
    double *y = (double *)((char *)workspace + 256);
    double *part = y + n;
    const int NB = eig_blocks(n);
    const double bound = (double)n * tol;
    hipLaunchKernelGGL(eig_init_kernel, dim3((unsigned)((n + RT - 1) / RT)), dim3(RT), 0, st, n, x_out, ctrl);
    for (int it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(eig_spmv_kernel, dim3(NB), dim3(RT), 0, st, n, row_ptr, col, (const double *)x_out, y, part, (const EigCtrl *)ctrl);
        hipLaunchKernelGGL(eig_norm_kernel, dim3(1), dim3(RT), 0, st, NB, (const double *)part, ctrl);
        hipLaunchKernelGGL(eig_scale_kernel, dim3(NB), dim3(RT), 0, st, n, (const double *)y, x_out, part, (const EigCtrl *)ctrl);
        hipLaunchKernelGGL(eig_test_kernel, dim3(1), dim3(RT), 0, st, NB, (const double *)part, bound, it + 1, ctrl);
    }
    CTGCN_TRY(hipGetLastError());
    EigCtrl h{};
    CTGCN_TRY(hipMemcpyAsync(&h, ctrl, sizeof(EigCtrl), hipMemcpyDeviceToHost, st));
    CTGCN_TRY(hipStreamSynchronize(st));
    *stop_step_host = h.done ? h.stop_step : 0;
    return CTGCN_OK;
}

static int check_ridge_args(const char *what, int64_t n, int32_t d, int32_t targets, int32_t folds, int64_t ldx, const void *X, const double *Y)
{
    char buf[192];
    if (d > RIDGE_MAXD || targets > RIDGE_MAXT) {
        snprintf(buf, sizeof(buf), "%s: unsupported shape (need d <= %d, targets <= %d)", what, RIDGE_MAXD, RIDGE_MAXT);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (n < 1 || d < 1 || targets < 1 || folds < 2 || folds > n || ldx < d) {
        snprintf(buf, sizeof(buf), "%s: bad sizes (need d >= 1, targets >= 1, 2 <= folds <= n, ldx >= d)", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    if (!X || !Y) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    return CTGCN_OK;
}

extern "C" size_t ctgcn_ridge_gram_workspace_bytes(int32_t d, int32_t targets, int32_t folds)
{
    if (d < 1 || targets < 1 || folds < 1) return 0;
    return sizeof(double) * (size_t)folds * RIDGE_CHUNKS * (d + 1) * (d + 1 + targets);
}

template <typename TX>
static int ridge_gram(int64_t n, int32_t d, int32_t targets, int32_t folds, const TX *X, int64_t ldx, const double *Y, double *gram_out,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_ridge_args("ridge_gram", n, d, targets, folds, ldx, X, Y);
    if (rc) return rc;
    if (!gram_out || !workspace) return ctgcn_set_error_(CTGCN_E_INVALID, "ridge_gram: null pointer");
    if (workspace_bytes < ctgcn_ridge_gram_workspace_bytes(d, targets, folds))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ridge_gram: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int NR = d + 1, NC = d + 1 + targets;
    const unsigned tiles = (unsigned)(((NR + GT - 1) / GT) * ((NC + GT - 1) / GT));
    double *part = (double *)workspace;
    hipLaunchKernelGGL(ridge_gram_kernel<TX>, dim3(tiles, folds * RIDGE_CHUNKS), dim3(RT), 0, st, n, (int)d, (int)targets, (int)folds, X, ldx,
                       Y, part);
    const int64_t per = (int64_t)NR * NC;
    hipLaunchKernelGGL(chunk_reduce_kernel, dim3((unsigned)((per + RT - 1) / RT), folds), dim3(RT), 0, st, per, RIDGE_CHUNKS,
                       (const double *)part, gram_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_ridge_gram_f32(int64_t n, int32_t d, int32_t targets, int32_t folds, const float *X, int64_t ldx, const double *Y,
                                    double *gram_out, void *workspace, size_t workspace_bytes, void *stream)
{
    return ridge_gram<float>(n, d, targets, folds, X, ldx, Y, gram_out, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_ridge_gram_f64(int64_t n, int32_t d, int32_t targets, int32_t folds, const double *X, int64_t ldx, const double *Y,
                                    double *gram_out, void *workspace, size_t workspace_bytes, void *stream)
{
    return ridge_gram<double>(n, d, targets, folds, X, ldx, Y, gram_out, workspace, workspace_bytes, stream);
}

extern "C" size_t ctgcn_ridge_sse_workspace_bytes(int32_t models, int32_t folds)
{
    if (models < 1 || folds < 1) return 0;
    return sizeof(double) * (size_t)folds * RIDGE_CHUNKS * SSE_SPLIT * models;
}

template <typename TX>
static int ridge_sse(int64_t n, int32_t d, int32_t targets, int32_t folds, int32_t models, const TX *X, int64_t ldx, const double *Y,
                     const double *W, const int32_t *target_of, double *sse_out, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_ridge_args("ridge_sse", n, d, targets, folds, ldx, X, Y);
    if (rc) return rc;
    if (models > RIDGE_MAXP) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "ridge_sse: more than 64 models");
    if (models < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "ridge_sse: models < 1");
    if (!W || !target_of || !sse_out || !workspace) return ctgcn_set_error_(CTGCN_E_INVALID, "ridge_sse: null pointer");
    if (workspace_bytes < ctgcn_ridge_sse_workspace_bytes(models, folds))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ridge_sse: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    hipLaunchKernelGGL(ridge_sse_kernel<TX>, dim3(SSE_SPLIT, folds * RIDGE_CHUNKS), dim3(RT), 0, st, n, (int)d, (int)targets, (int)folds, (int)models,
                       X, ldx, Y, W, (const int *)target_of, part);
    hipLaunchKernelGGL(chunk_reduce_kernel, dim3(1, folds), dim3(RT), 0, st, (int64_t)models, RIDGE_CHUNKS * SSE_SPLIT, (const double *)part,
                       sse_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_ridge_sse_f32(int64_t n, int32_t d, int32_t targets, int32_t folds, int32_t models, const float *X, int64_t ldx,
                                   const double *Y, const double *W, const int32_t *target_of, double *sse_out, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return ridge_sse<float>(n, d, targets, folds, models, X, ldx, Y, W, target_of, sse_out, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_ridge_sse_f64(int64_t n, int32_t d, int32_t targets, int32_t folds, int32_t models, const double *X, int64_t ldx,
                                   const double *Y, const double *W, const int32_t *target_of, double *sse_out, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    return ridge_sse<double>(n, d, targets, folds, models, X, ldx, Y, W, target_of, sse_out, workspace, workspace_bytes, stream);
}
