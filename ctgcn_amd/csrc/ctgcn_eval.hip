// ctgcn_eval.hip — link-prediction evaluation (reference evaluation/link_prediction.py) on the GPU.
//
//   - lp_neg_sample_kernel: the negative edges of all three splits in one launch.  Slot s draws uniform ordered pairs keyed on
//     (seed, s, attempt) until one has u != v and neither (u, v) nor (v, u) in the sorted membership keys u·N + v: the output
//     depends on (seed, slot) only, never on the launch configuration.  Attempts are capped; a slot that hits the cap raises a flag.
//   - lp_pass_kernel<GRAD>: one pass over an edge set for up to 16 logistic-regression models at once.  Each 32-edge tile gathers
//     the two embedding rows of every edge into LDS once; the features (Avg, Had, L1, L2) are formed in registers from those rows
//     and never stored.  GRAD: Σ s_i·logloss and Σ s_i (σ(z_i) - y_i) (φ_i, 1) per model (fp32 inside a tile, fp64 across tiles);
//     otherwise the scores z = w·φ + b.
//   - lp_hess_kernel<MAXB>: Σ s_i σ(1-σ) (φ_i, 1)(φ_i, 1)ᵀ per model, fp32 over one part of the edges, upper triangle only.
// No float atomics anywhere: per-block partials are summed in a fixed order by lp_reduce_kernel, so repeated calls are bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "ctgcn_logreg.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr int THREADS = 256;
constexpr int TE = 32;               // edges per tile
constexpr int MAXM = 16;             // models per pass
constexpr int MAXD = 256;
constexpr int MAX_GRID = 1024;       // pass blocks (grid-stride over tiles); depends on n only, so the reduction order is fixed
constexpr int HESS_PARTS = 64;

__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// measure ids: 0 Avg (a+b)/2, 1 Had a*b, 2 L1 |a-b|, 3 L2 (a-b)^2
__device__ __forceinline__ float feature(int meas, float a, float b)
{
    const float df = a - b;
    return (meas & 2) ? ((meas & 1) ? df * df : fabsf(df)) : ((meas & 1) ? a * b : 0.5f * (a + b));
}

__device__ __forceinline__ bool key_found(const int64_t *__restrict__ keys, int64_t n_keys, int64_t k)
{
    int64_t lo = 0, hi = n_keys;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < n_keys && keys[lo] == k;
}

__global__ __launch_bounds__(THREADS) void lp_neg_sample_kernel(int64_t count, int64_t n_nodes, const int64_t *__restrict__ keys,
                                                                int64_t n_keys, uint64_t seed, int64_t max_attempts,
                                                                int64_t *__restrict__ from_out, int64_t *__restrict__ to_out,
                                                                int32_t *__restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (s >= count) return;
    for (int64_t k = 0; k < max_attempts; ++k) {
        int64_t u = (int64_t)(ctgcn_u01(seed, (uint64_t)s, (uint64_t)(2 * k)) * (double)n_nodes);
        int64_t v = (int64_t)(ctgcn_u01(seed, (uint64_t)s, (uint64_t)(2 * k + 1)) * (double)n_nodes);
        u = min(u, n_nodes - 1);
        v = min(v, n_nodes - 1);
        if (u == v || key_found(keys, n_keys, u * n_nodes + v) || key_found(keys, n_keys, v * n_nodes + u)) continue;
        from_out[s] = u;
        to_out[s] = v;
        return;
    }
    from_out[s] = -1;
    to_out[s] = -1;
    *flag = 1;
}

// LDS row stride of the gathered embedding rows: odd, so a column read across 32 edges hits 32 distinct banks
__host__ __device__ __forceinline__ int row_stride(int d) { return d | 1; }

// Gather the source rows (LDS rows 0..TE-1) and destination rows (TE..2TE-1) of tile edges [e0, e0 + TE); rows past n are zero.
__device__ __forceinline__ void gather_tile(float *X, int S, int64_t e0, int64_t n, int d, int64_t n_nodes, const float *__restrict__ E,
                                            int64_t lde, const int64_t *__restrict__ src, const int64_t *__restrict__ dst)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < 2 * TE; r += THREADS / 64) {
        const int64_t e = e0 + (r % TE);
        int64_t node = -1;
        if (e < n) node = r < TE ? src[e] : dst[e];
        float *out = X + r * S;
        if (node >= 0 && node < n_nodes) {
            const float *row = E + node * lde;
            for (int c = lane; c < d; c += 64) out[c] = row[c];
        } else {
            for (int c = lane; c < d; c += 64) out[c] = 0.f;
        }
    }
}

// One pass over n edges for M models; W: fp32 [2, M, d+1] (w then b): the parameters as hi + lo, so z sees a double-precision
// iterate without a systematic fp32 rounding of w (the rounding of the fp32 accumulation itself averages out over the edges).  GRAD: block partials [grad M*(d+1) | loss M] (double) into part;
// otherwise score[m * n + e] = z.
template <bool GRAD>
__global__ __launch_bounds__(THREADS) void lp_pass_kernel(int64_t n, int d, int M, uint32_t measures, int64_t n_nodes, const float *__restrict__ E,
                                                          int64_t lde, const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                                                          const uint8_t *__restrict__ label, double w_neg, double w_pos,
                                                          const float *__restrict__ W, double *__restrict__ part, float *__restrict__ score)
{
    extern __shared__ float sm[];
    const int S = row_stride(d), D1 = d + 1;
    float *X = sm;                       // [2 TE, S]
    float *Wl = X + 2 * TE * S;          // [2, M, D1]
    float *R = Wl + 2 * M * D1;          // [M, TE]: s_i (σ(z_i) - y_i) of the tile
    const float *Wlo = Wl + M * D1;
    const int t = threadIdx.x;
    for (int i = t; i < 2 * M * D1; i += THREADS) Wl[i] = W[i];

    // phase 1 / 2 mapping: edge e1 of the tile, models q and q + 8
    const int e1 = t & (TE - 1), q = t >> 5;
    // phase 3 mapping: column j, model group g owning models [g·KM, (g+1)·KM)
    const int ngroups = d <= 64 ? 4 : (d <= 128 ? 2 : 1);
    const int cw = THREADS / ngroups, j = t % cw, g = t / cw;
    const int KM = (M + ngroups - 1) / ngroups;
    double gacc[MAXM];
    int gmeas[MAXM];
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
        gacc[k] = 0.0;
        const int m = g * KM + k;
        gmeas[k] = m < M ? (int)((measures >> (2 * m)) & 3u) : 0;
    }
    double lacc[2] = {0.0, 0.0}, racc[2] = {0.0, 0.0};
    int qmeas[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) qmeas[h] = (int)((measures >> (2 * (q + 8 * h))) & 3u);

    const int64_t ntiles = ceil_div(n, TE);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t e0 = tile * TE;
        __syncthreads();                 // the previous tile's phase 3 is done with X and R
        gather_tile(X, S, e0, n, d, n_nodes, E, lde, src, dst);
        __syncthreads();
        const float *xa = X + e1 * S, *xb = X + (TE + e1) * S;
        float z[2] = {0.f, 0.f}, zl[2] = {0.f, 0.f};
        for (int c = 0; c < d; ++c) {
            const float a = xa[c], b = xb[c];
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (q + 8 * h < M) {
                    const float f = feature(qmeas[h], a, b);
                    z[h] += f * Wl[(q + 8 * h) * D1 + c];
                    zl[h] += f * Wlo[(q + 8 * h) * D1 + c];
                }
        }
        const int64_t e = e0 + e1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = q + 8 * h;
            if (m >= M) continue;
            const float zm = (z[h] + Wl[m * D1 + d]) + (zl[h] + Wlo[m * D1 + d]);
            if (!GRAD) {
                if (e < n) score[(int64_t)m * n + e] = zm;
                continue;
            }
            double r = 0.0;
            if (e < n) {
                const bool y = label[e] != 0;
                const double s = y ? w_pos : w_neg, zd = (double)zm;
                lacc[h] += s * softplus(y ? -zd : zd);
                r = s * (sigmoid(zd) - (y ? 1.0 : 0.0));
                racc[h] += r;
            }
            R[m * TE + e1] = (float)r;
        }
        if (!GRAD) continue;
        __syncthreads();
        if (j < d) {
            float acc[MAXM];
#pragma unroll
            for (int k = 0; k < MAXM; ++k) acc[k] = 0.f;
            for (int ee = 0; ee < TE; ++ee) {
                const float a = X[ee * S + j], b = X[(TE + ee) * S + j];
#pragma unroll
                for (int k = 0; k < MAXM; ++k)
                    if (k < KM && g * KM + k < M) acc[k] += R[(g * KM + k) * TE + ee] * feature(gmeas[k], a, b);
            }
#pragma unroll
            for (int k = 0; k < MAXM; ++k) gacc[k] += (double)acc[k];
        }
    }
    if (!GRAD) return;
    const int64_t stride = (int64_t)M * D1 + M;
    double *out = part + blockIdx.x * stride;
    if (j < d) {
#pragma unroll
        for (int k = 0; k < MAXM; ++k)
            if (k < KM && g * KM + k < M) out[(g * KM + k) * D1 + j] = gacc[k];
    }
    // intercept gradient and loss: fixed-order butterfly over the 32 edge lanes of each half wave
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        double l = lacc[h], r = racc[h];
#pragma unroll
        for (int o = 1; o < TE; o <<= 1) {
            l += __shfl_xor(l, o, 64);
            r += __shfl_xor(r, o, 64);
        }
        const int m = q + 8 * h;
        if (e1 == 0 && m < M) {
            out[m * D1 + d] = r;
            out[(int64_t)M * D1 + m] = l;
        }
    }
}

// Hessian partials: block (p, m) covers edges [p·chunk, min((p+1)·chunk, n)); part[(p·M + m)·D1² + j·D1 + k] for j <= k.
template <int MAXB>
__global__ __launch_bounds__(THREADS) void lp_hess_kernel(int64_t n, int64_t chunk, int d, int M, uint32_t measures, int64_t n_nodes,
                                                          const float *__restrict__ E, int64_t lde, const int64_t *__restrict__ src,
                                                          const int64_t *__restrict__ dst, const uint8_t *__restrict__ label, double w_neg,
                                                          double w_pos, const float *__restrict__ W, float *__restrict__ part)
{
    extern __shared__ float sm[];
    const int D1 = d + 1, D4 = (D1 + 3) & ~3, nb = D4 / 4, ntri = nb * (nb + 1) / 2;
    float *F = sm;                       // [TE, D4]: (φ, 1, 0...)
    float *Aw = F + TE * D4;             // [TE]: s σ(1-σ)
    const int p = blockIdx.x, m = blockIdx.y, t = threadIdx.x;
    const int meas = (int)((measures >> (2 * m)) & 3u);
    const float *w = W + (int64_t)m * D1;
    int bj[MAXB], bk[MAXB];
    float acc[MAXB][16];
    hess_blocks<MAXB, THREADS>(nb, ntri, bj, bk, acc);

    const int64_t lo = (int64_t)p * chunk, hi = min(n, lo + chunk);
    const int wave = t >> 6, lane = t & 63;
    for (int64_t e0 = lo; e0 < hi; e0 += TE) {
        __syncthreads();
        for (int r = wave; r < TE; r += THREADS / 64) {
            const int64_t e = e0 + r;
            const int64_t u = e < hi ? src[e] : -1, v = e < hi ? dst[e] : -1;
            const bool ok = u >= 0 && u < n_nodes && v >= 0 && v < n_nodes;
            for (int c = lane; c < D4; c += 64) {
                float f = 0.f;
                if (ok && c < d) f = feature(meas, E[u * lde + c], E[v * lde + c]);
                else if (ok && c == d) f = 1.f;
                F[r * D4 + c] = f;
            }
        }
        __syncthreads();
        const float zp = hess_row_z(F, D4, D1, w);
        if ((t & 7) == 0) {
            const int64_t e = e0 + (t >> 3);
            Aw[t >> 3] = e < hi ? hess_curvature(label[e] ? w_pos : w_neg, zp) : 0.f;
        }
        __syncthreads();
        hess_accumulate<MAXB, TE>(F, D4, Aw, bj, bk, acc);
    }
    hess_store_upper<MAXB>(part + ((int64_t)p * M + m) * D1 * D1, D1, bj, bk, acc);
}

// out[v] = Σ_b part[b·stride + v] in block order (fp64)
__global__ __launch_bounds__(THREADS) void lp_reduce_kernel(int64_t count, int64_t blocks, int64_t stride, const double *__restrict__ part,
                                                            double *__restrict__ out)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= count) return;
    double s = 0.0;
    for (int64_t b = 0; b < blocks; ++b) s += part[b * stride + v];
    out[v] = s;
}

// hess[m][j][k] = Σ_p part[p][m][min(j,k)][max(j,k)] in part order (fp64), both triangles
__global__ __launch_bounds__(THREADS) void lp_hess_reduce_kernel(int M, int D1, int parts, const float *__restrict__ part, double *__restrict__ hess)
{
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t per = (int64_t)D1 * D1;
    if (v >= (int64_t)M * per) return;
    const int m = (int)(v / per), r = (int)(v % per), j = r / D1, k = r % D1;
    const int64_t off = (int64_t)m * per + (int64_t)min(j, k) * D1 + max(j, k);
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += (double)part[(int64_t)p * M * per + off];
    hess[v] = s;
}

int64_t pass_blocks(int64_t n) { return n <= 0 ? 0 : std::min<int64_t>((n + TE - 1) / TE, MAX_GRID); }
size_t pass_lds(int d, int M) { return sizeof(float) * ((size_t)2 * TE * row_stride(d) + (size_t)2 * M * (d + 1) + (size_t)M * TE); }
int hess_parts(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(HESS_PARTS, (n + 4 * TE - 1) / (4 * TE))); }

}  // namespace

static int check_pass_args(const char *what, int64_t n, int32_t d, int32_t models, int64_t n_nodes, const float *E, int64_t lde,
                           const int64_t *src, const int64_t *dst, const float *W)
{
    char buf[160];
    if (n < 0 || d < 1 || d > MAXD || models < 1 || models > MAXM || n_nodes < 1 || lde < d) {
        snprintf(buf, sizeof(buf), "%s: bad sizes (need n >= 0, 1 <= d <= %d, 1 <= models <= %d, lde >= d)", what, MAXD, MAXM);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    if (n > 0 && (!E || !src || !dst || !W)) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    return CTGCN_OK;
}

extern "C" int ctgcn_lp_neg_sample(int64_t count, int64_t n_nodes, const int64_t *keys, int64_t n_keys, uint64_t seed, int64_t max_attempts,
                                   int64_t *from_out, int64_t *to_out, int32_t *flag, void *stream)
{
    if (count < 0 || n_nodes < 2 || n_keys < 0 || max_attempts < 1 || n_nodes > 3037000499LL)
        return ctgcn_set_error_(CTGCN_E_INVALID, "lp_neg_sample: bad sizes (need n_nodes in [2, 3037000499], max_attempts >= 1)");
    if (count == 0) return CTGCN_OK;
    if (!from_out || !to_out || !flag || (n_keys > 0 && !keys)) return ctgcn_set_error_(CTGCN_E_INVALID, "lp_neg_sample: null pointer");
    if ((count + THREADS - 1) / THREADS > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "lp_neg_sample: count too large");
    hipStream_t st = (hipStream_t)stream;
    CTGCN_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(lp_neg_sample_kernel, dim3((unsigned)((count + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, count, n_nodes, keys,
                       n_keys, seed, max_attempts, from_out, to_out, flag);
    CTGCN_TRY(hipGetLastError());
    int32_t hit = 0;
    CTGCN_TRY(hipMemcpyAsync(&hit, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CTGCN_TRY(hipStreamSynchronize(st));
    if (hit) return ctgcn_set_error_(CTGCN_E_LIMIT, "lp_neg_sample: a slot reached max_attempts without a valid negative pair");
    return CTGCN_OK;
}

extern "C" size_t ctgcn_lp_grad_workspace_bytes(int64_t n, int32_t d, int32_t models)
{
    if (n < 0 || d < 1 || models < 1) return 0;
    return (size_t)pass_blocks(n) * ((size_t)models * (d + 1) + models) * sizeof(double);
}

extern "C" int ctgcn_lp_grad_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                                 const int64_t *src, const int64_t *dst, const uint8_t *label, double w_neg, double w_pos, const float *W,
                                 double *loss_out, double *grad_out, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_pass_args("lp_grad", n, d, models, n_nodes, E, lde, src, dst, W);
    if (rc) return rc;
    if (!loss_out || !grad_out || (n > 0 && (!label || !workspace))) return ctgcn_set_error_(CTGCN_E_INVALID, "lp_grad: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t D1 = d + 1, stride = (int64_t)models * D1 + models;
    if (n == 0) {
        CTGCN_TRY(hipMemsetAsync(grad_out, 0, sizeof(double) * models * D1, st));
        CTGCN_TRY(hipMemsetAsync(loss_out, 0, sizeof(double) * models, st));
        return CTGCN_OK;
    }
    if (workspace_bytes < ctgcn_lp_grad_workspace_bytes(n, d, models)) return ctgcn_set_error_(CTGCN_E_WORKSPACE, "lp_grad: workspace too small");
    const int64_t blocks = pass_blocks(n);
    double *part = (double *)workspace;
    rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(lp_pass_kernel<true>), pass_lds(d, models), "lp_grad");
    if (rc) return rc;
    hipLaunchKernelGGL(lp_pass_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), pass_lds(d, models), st, n, (int)d, (int)models, measures,
                       n_nodes, E, lde, src, dst, label, w_neg, w_pos, W, part, (float *)nullptr);
    const int64_t ng = (int64_t)models * D1;
    hipLaunchKernelGGL(lp_reduce_kernel, dim3((unsigned)((ng + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, ng, blocks, stride,
                       (const double *)part, grad_out);
    hipLaunchKernelGGL(lp_reduce_kernel, dim3(1), dim3(THREADS), 0, st, (int64_t)models, blocks, stride, (const double *)(part + ng), loss_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_lp_scores_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                                   const int64_t *src, const int64_t *dst, const float *W, float *score_out, void *stream)
{
    int rc = check_pass_args("lp_scores", n, d, models, n_nodes, E, lde, src, dst, W);
    if (rc) return rc;
    if (n == 0) return CTGCN_OK;
    if (!score_out) return ctgcn_set_error_(CTGCN_E_INVALID, "lp_scores: null pointer");
    hipStream_t st = (hipStream_t)stream;
    rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(lp_pass_kernel<false>), pass_lds(d, models), "lp_scores");
    if (rc) return rc;
    hipLaunchKernelGGL(lp_pass_kernel<false>, dim3((unsigned)pass_blocks(n)), dim3(THREADS), pass_lds(d, models), st, n, (int)d, (int)models,
                       measures, n_nodes, E, lde, src, dst, (const uint8_t *)nullptr, 0.0, 0.0, W, (double *)nullptr, score_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_lp_hess_workspace_bytes(int64_t n, int32_t d, int32_t models)
{
    if (n < 0 || d < 1 || models < 1) return 0;
    return (size_t)hess_parts(n) * models * (size_t)(d + 1) * (d + 1) * sizeof(float);
}

extern "C" int ctgcn_lp_hess_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                                 const int64_t *src, const int64_t *dst, const uint8_t *label, double w_neg, double w_pos, const float *W,
                                 double *hess_out, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_pass_args("lp_hess", n, d, models, n_nodes, E, lde, src, dst, W);
    if (rc) return rc;
    if (!hess_out || (n > 0 && (!label || !workspace))) return ctgcn_set_error_(CTGCN_E_INVALID, "lp_hess: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int D1 = d + 1;
    const int64_t total = (int64_t)models * D1 * D1;
    if (n == 0) {
        CTGCN_TRY(hipMemsetAsync(hess_out, 0, sizeof(double) * total, st));
        return CTGCN_OK;
    }
    if (workspace_bytes < ctgcn_lp_hess_workspace_bytes(n, d, models)) return ctgcn_set_error_(CTGCN_E_WORKSPACE, "lp_hess: workspace too small");
    const int parts = hess_parts(n);
    const int64_t chunk = (n + parts - 1) / parts;
    const int D4 = (D1 + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)TE * D4 + TE);
    float *part = (float *)workspace;
    if (d <= 128)        // (d+1) padded to 4: at most 33 column blocks, 561 upper-triangle tiles -> 3 per thread
        hipLaunchKernelGGL(lp_hess_kernel<3>, dim3(parts, models), dim3(THREADS), lds, st, n, chunk, (int)d, (int)models, measures, n_nodes, E,
                           lde, src, dst, label, w_neg, w_pos, W, part);
    else                 // at most 65 column blocks, 2145 tiles -> 9 per thread
        hipLaunchKernelGGL(lp_hess_kernel<9>, dim3(parts, models), dim3(THREADS), lds, st, n, chunk, (int)d, (int)models, measures, n_nodes, E,
                           lde, src, dst, label, w_neg, w_pos, W, part);
    hipLaunchKernelGGL(lp_hess_reduce_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (int)models, D1, parts,
                       (const float *)part, hess_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
