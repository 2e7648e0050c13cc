// ctgcn_nodecls.hip — node-classification evaluation (reference evaluation/node_classification.py) on the GPU.
//
// A launch covers a batch of independent one-vs-rest problems described by a problem table (include/ctgcn_hip.h):
//   - nc_pass_kernel<false>: Σ s_i·logloss and Σ s_i (σ(z_i) - y_i) (x_i, 1) of every model.  Each 32-row tile of a problem is
//     gathered into LDS once, with the bias column 1 appended, and serves every model of its block (up to 64 models: all of a
//     problem's models unless it has more).  fp32 inside a tile, fp64 across tiles.
//   - nc_pass_kernel<true>: the same tile pass gives z of every model, then the predicted class of every row for every C group
//     (first argmax of fp64 expit(z), constant models contributing their constant) and integer correct counts per (problem, C).
//   - nc_hess_kernel<MAXB>: Σ s_i σ(1-σ) (x_i, 1)(x_i, 1)ᵀ per model over a strided subsample of its problem, upper triangle.
// No float atomics: a problem's blocks are (problem, chunk) pairs whose count is a function of that problem's row count alone, and
// their fp64 partials are summed in chunk order by the reduce kernels.  So a problem's outputs are bit-identical across calls and do
// not depend on which other problems share the launch.
//
// Edge classification (reference evaluation/edge_classification.py) runs through the same kernels with a pair table: a second index
// array rows2 parallel to rows, the feature of entry i being E[rows[i]] ⊙ E[rows2[i]].  The product is formed while the tile is
// staged (gather_tile<true>), so no [edges, d] matrix exists; everything after the staging is the one body both kinds share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "ctgcn_logreg.h"
#include "ctgcn_try.h"

namespace {

constexpr int THREADS = 256;
constexpr int TE = 32;                 // rows per tile
constexpr int MAXD = 256;
constexpr int MAX_CHUNKS = 1024;       // pass blocks per problem (grid-stride over its tiles)
constexpr int MIN_TILES_PER_CHUNK = 4;
constexpr int HESS_ROWS_PER_PART = 1024;
constexpr int MAX_HESS_PARTS = 64;
constexpr int PAIRS = 9;               // (model, column quad) pairs per thread in the gradient phase: 64 x 33 or 32 x 65 <= 9 x 256

// models per block: 64 while a tile row (d+1 padded) fits 132 floats, 32 up to d = 256
__host__ __device__ __forceinline__ int group_max(int d) { return d + 1 <= 132 ? 64 : 32; }
// LDS row stride of tiles and parameters: d+1 rounded up to 4, with an odd number of 16-byte slots, so float4 reads of 16 distinct
// rows hit distinct bank quads
__host__ __device__ __forceinline__ int wstride(int d)
{
    int w = (d + 1 + 3) & ~3;
    if (((w >> 2) & 1) == 0) w += 4;
    return w;
}
__host__ __device__ __forceinline__ int64_t chunks_of(int64_t n)
{
    if (n <= 0) return 1;
    const int64_t c = (n + (int64_t)MIN_TILES_PER_CHUNK * TE - 1) / ((int64_t)MIN_TILES_PER_CHUNK * TE);
    return c < MAX_CHUNKS ? c : MAX_CHUNKS;
}
__host__ __device__ __forceinline__ int64_t hess_step(int64_t n, int64_t hess_max) { return n <= hess_max ? 1 : (n + hess_max - 1) / hess_max; }
__host__ __device__ __forceinline__ int64_t hess_rows(int64_t n, int64_t hess_max) { return n <= 0 ? 0 : (n + hess_step(n, hess_max) - 1) / hess_step(n, hess_max); }
__host__ __device__ __forceinline__ int64_t hess_parts_of(int64_t n, int64_t hess_max)
{
    const int64_t c = (hess_rows(n, hess_max) + HESS_ROWS_PER_PART - 1) / HESS_ROWS_PER_PART;
    return c < 1 ? 1 : (c < MAX_HESS_PARTS ? c : MAX_HESS_PARTS);
}

// largest i in [0, count) with start[i] <= v (start non-decreasing, start[0] <= v)
template <typename T>
__device__ __forceinline__ int find_slot(const T *__restrict__ start, int count, int64_t v)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)start[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Table {
    int P;
    const int64_t *row_start;    // [P+1]: rows / y entries of problem p
    const int64_t *block_start;  // [P+1]: chunk (pass) or part (Hessian) blocks of problem p
    const int64_t *rows;         // embedding row of each entry
    const int64_t *rows2;        // pair tables: the entry's second embedding row (its feature is the product of the two); else null
    int vec4;                    // pair tables: d % 4 == 0, lde % 4 == 0 and E 16-byte aligned, so rows are staged as float4
    const int32_t *y;            // class index of each entry
    const int32_t *model_start;  // [P+1]: models of problem p (the model arrays below are indexed relative to model_start[0])
    const int32_t *model_pos;    // positive class of each model
    const double *model_w;       // [M, 2]: balanced weights (negative, positive)
    const int32_t *model_flag;   // 0 fitted, 1 constant 0, 2 constant 1
};

// X [TE, DW]: row r = (x, 1, 0 ...) for i0 + r < cnt, zero otherwise, entry e = base + (i0 + r)·step.  x = E[rows[e]], or with PAIR
// E[rows[e]] ⊙ E[rows2[e]] (one fp32 multiply per column).  An index outside [0, n_emb) makes x zero.
// PAIR with tb.vec4: half a wave per row, a float4 per lane; a wave's 8 rows are 4 per half, and the index loads and then the row
// loads of both endpoints of all 4 are issued before the first LDS write.  Both PAIR paths write the same fp32 values.
template <bool PAIR>
__device__ __forceinline__ void gather_tile(float *X, int DW, int d, const Table &tb, int64_t base, int64_t step, int64_t i0, int64_t cnt,
                                            int64_t n_emb, const float *__restrict__ E, int64_t lde)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t *__restrict__ rows = tb.rows;
    if (PAIR && tb.vec4) {
        constexpr int RW = TE / (THREADS / 64) / 2;        // rows per half wave
        const int64_t *__restrict__ rows2 = tb.rows2;
        const int half = lane >> 5, hl = lane & 31, NQ = DW >> 2, dq = d >> 2;
        // every load below is unconditional (an entry past cnt reads entry i0, an index out of range reads row 0, and the value is
        // dropped): a load under a lane condition gets a wait of its own, which would put the rows in flight one at a time
        int64_t a[RW], b[RW];
        bool ok[RW], valid[RW];
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            const int64_t i = i0 + wave * (2 * RW) + 2 * k + half;
            ok[k] = i < cnt;
            const int64_t e = base + (ok[k] ? i : i0) * step;
            a[k] = rows[e];
            b[k] = rows2[e];
        }
#pragma unroll
        for (int k = 0; k < RW; ++k) {
            valid[k] = ok[k] && a[k] >= 0 && a[k] < n_emb && b[k] >= 0 && b[k] < n_emb;
            a[k] = valid[k] ? a[k] : 0;
            b[k] = valid[k] ? b[k] : 0;
        }
        for (int q = hl; q < dq; q += 32) {
            float4 va[RW], vb[RW];
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                va[k] = *reinterpret_cast<const float4 *>(E + a[k] * lde + 4 * q);
                vb[k] = *reinterpret_cast<const float4 *>(E + b[k] * lde + 4 * q);
            }
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                float4 o = make_float4(va[k].x * vb[k].x, va[k].y * vb[k].y, va[k].z * vb[k].z, va[k].w * vb[k].w);
                if (!valid[k]) o = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(X + (wave * (2 * RW) + 2 * k + half) * DW + 4 * q) = o;
            }
        }
        if (dq + hl < NQ)                                  // the bias quad and the padding after it
#pragma unroll
            for (int k = 0; k < RW; ++k)
                *reinterpret_cast<float4 *>(X + (wave * (2 * RW) + 2 * k + half) * DW + 4 * (dq + hl)) =
                    make_float4(hl == 0 && ok[k] ? 1.f : 0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (int r = wave; r < TE; r += THREADS / 64) {
        const int64_t i = i0 + r;
        const bool ok = i < cnt;
        const int64_t node = ok ? rows[base + i * step] : -1;
        const int64_t node2 = PAIR ? (ok ? tb.rows2[base + i * step] : -1) : 0;
        const bool valid = node >= 0 && node < n_emb && node2 >= 0 && node2 < n_emb;
        float *out = X + r * DW;
        for (int c = lane; c < DW; c += 64) {
            float v = 0.f;
            if (valid && c < d) v = PAIR ? E[node * lde + c] * E[node2 * lde + c] : E[node * lde + c];
            else if (ok && c == d) v = 1.f;
            out[c] = v;
        }
    }
}

// One pass over the rows of every problem.  Block (blockIdx.x = chunk block b of problem p, blockIdx.y = model block g).
//   GRAD (PREDICT false): models [g·gm, (g+1)·gm) of p; part[(b·G + g)·(gm·DW + gm) ...]: gradient [gm, DW] then loss [gm] (fp64).
//   PREDICT: C groups [g·gpb, (g+1)·gpb) of p (gpb = gm / models per group); pred_out[(entry - row_start[0])·groups + group] and
//   correct_out[p·groups + group] (integer atomics: exact, order-free).
template <bool PREDICT, bool PAIR>
__global__ __launch_bounds__(THREADS) void nc_pass_kernel(Table tb, int d, int gm, int groups, const int32_t *__restrict__ n_classes,
                                                          int64_t n_emb, const float *__restrict__ E, int64_t lde, const float *__restrict__ W,
                                                          int64_t M, double *__restrict__ part, int32_t *__restrict__ pred_out,
                                                          unsigned long long *__restrict__ correct_out)
{
    extern __shared__ double smd[];
    const int DW = wstride(d), D1 = d + 1, t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int p = find_slot(tb.block_start, tb.P + 1, b);
    const int64_t nch = tb.block_start[p + 1] - tb.block_start[p], c0 = b - tb.block_start[p];
    const int64_t rs = tb.row_start[p], n = tb.row_start[p + 1] - rs;
    const int64_t ms = tb.model_start[p] - tb.model_start[0], me = tb.model_start[p + 1] - tb.model_start[0];
    int64_t m0, cnt;
    int mpg = 1, gpb = 0, gi0 = 0;
    if (PREDICT) {
        const int K = n_classes[p];
        mpg = K <= 2 ? 1 : K;
        gpb = gm / mpg;
        gi0 = blockIdx.y * gpb;
        const int gi1 = min(gi0 + gpb, groups);
        m0 = ms + (int64_t)gi0 * mpg;
        cnt = min((int64_t)(gi1 - gi0) * mpg, me - m0);
    } else {
        m0 = ms + (int64_t)blockIdx.y * gm;
        cnt = min((int64_t)gm, me - m0);
    }
    if (cnt <= 0) return;                                  // uniform over the block

    double *Ld = smd;                                      // [THREADS]
    float *X = reinterpret_cast<float *>(smd + THREADS);   // [TE, DW]
    float *Wl = X + TE * DW;                               // [2, gm, DW]: hi then lo
    float *R = Wl + 2 * gm * DW;                           // [gm, TE]: GRAD s(σ - y), PREDICT z
    for (int i = t; i < 2 * gm * DW; i += THREADS) {
        const int h = i / (gm * DW), rem = i % (gm * DW), k = rem / DW, c = rem % DW;
        Wl[i] = (k < cnt && c < D1) ? W[(int64_t)h * M * D1 + (m0 + k) * D1 + c] : 0.f;
    }

    // z phase: model lane mk, rows rg + RG·k (RG·RPT = TE)
    const int ML = cnt <= 8 ? 8 : (cnt <= 16 ? 16 : (cnt <= 32 ? 32 : 64));
    const int RG = THREADS / ML, RPT = TE / RG, mk = t % ML, rg = t / ML;
    int32_t flag = 1, pos = 0;
    double w_neg = 0.0, w_pos = 0.0;
    if (!PREDICT && mk < cnt) {
        flag = tb.model_flag[m0 + mk];
        pos = tb.model_pos[m0 + mk];
        w_neg = tb.model_w[2 * (m0 + mk)];
        w_pos = tb.model_w[2 * (m0 + mk) + 1];
    }
    double lacc = 0.0;
    // gradient phase: pairs (model mm, column quad q), flattened with stride THREADS
    const int NQ = DW / 4;
    double gacc[PAIRS][4];
#pragma unroll
    for (int k = 0; k < PAIRS; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) gacc[k][c] = 0.0;
    __shared__ unsigned int hits[64];
    if (PREDICT && t < 64) hits[t] = 0u;

    const int64_t ntiles = (n + TE - 1) / TE;
    for (int64_t tile = c0; tile < ntiles; tile += nch) {
        const int64_t i0 = tile * TE;
        __syncthreads();                                   // the previous tile is done with X and R (first pass: Wl, hits written)
        gather_tile<PAIR>(X, DW, d, tb, rs, 1, i0, n, n_emb, E, lde);
        __syncthreads();
        float z[8], zl[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = zl[k] = 0.f;
        if (mk < cnt) {
            const float4 *wh = reinterpret_cast<const float4 *>(Wl + mk * DW);
            const float4 *wo = reinterpret_cast<const float4 *>(Wl + (gm + mk) * DW);
            for (int q = 0; q < NQ; ++q) {
                const float4 a = wh[q], o = wo[q];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < RPT) {
                        const float4 x = *reinterpret_cast<const float4 *>(X + (rg + RG * k) * DW + 4 * q);
                        z[k] = fmaf(x.x, a.x, z[k]);
                        z[k] = fmaf(x.y, a.y, z[k]);
                        z[k] = fmaf(x.z, a.z, z[k]);
                        z[k] = fmaf(x.w, a.w, z[k]);
                        zl[k] = fmaf(x.x, o.x, zl[k]);
                        zl[k] = fmaf(x.y, o.y, zl[k]);
                        zl[k] = fmaf(x.z, o.z, zl[k]);
                        zl[k] = fmaf(x.w, o.w, zl[k]);
                    }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < RPT) {
                    const int r = rg + RG * k;
                    const int64_t i = i0 + r;
                    const float zm = z[k] + zl[k];
                    if (PREDICT) {
                        R[mk * TE + r] = zm;
                        continue;
                    }
                    double res = 0.0;
                    if (i < n && flag == 0) {
                        const bool yv = tb.y[rs + i] == pos;
                        const double s = yv ? w_pos : w_neg, zd = (double)zm;
                        lacc += s * softplus(yv ? -zd : zd);
                        res = s * (sigmoid(zd) - (yv ? 1.0 : 0.0));
                    }
                    R[mk * TE + r] = (float)res;
                }
        }
        __syncthreads();
        if (PREDICT) {
            const int ng = (int)(cnt / mpg);
            for (int u = t; u < ng * TE; u += THREADS) {
                const int r = u % TE, gl = u / TE;
                const int64_t i = i0 + r;
                if (i >= n) continue;
                int best = 0;
                double bp = -1.0;
                for (int k = 0; k < mpg; ++k) {
                    const int mm = gl * mpg + k;
                    const int32_t fl = tb.model_flag[m0 + mm];
                    const double pr = fl == 1 ? 0.0 : (fl == 2 ? 1.0 : sigmoid((double)R[mm * TE + r]));
                    if (mpg == 1) best = pr > 1.0 - pr ? 1 : 0;
                    else if (k == 0 || pr > bp) { best = k; bp = pr; }
                }
                pred_out[(rs - tb.row_start[0] + i) * groups + gi0 + gl] = best;
                if (best == tb.y[rs + i]) atomicAdd(&hits[gl], 1u);
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) {
            const int pi = t + THREADS * k, mm = pi / NQ, q = pi % NQ;
            if (mm < cnt) {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                for (int r = 0; r < TE; ++r) {
                    const float rv = R[mm * TE + r];
                    const float4 x = *reinterpret_cast<const float4 *>(X + r * DW + 4 * q);
                    a0 = fmaf(rv, x.x, a0);
                    a1 = fmaf(rv, x.y, a1);
                    a2 = fmaf(rv, x.z, a2);
                    a3 = fmaf(rv, x.w, a3);
                }
                gacc[k][0] += (double)a0;
                gacc[k][1] += (double)a1;
                gacc[k][2] += (double)a2;
                gacc[k][3] += (double)a3;
            }
        }
    }
    if (PREDICT) {
        __syncthreads();
        const int ng = (int)(cnt / mpg);
        if (t < ng && hits[t]) atomicAdd(correct_out + (int64_t)p * groups + gi0 + t, (unsigned long long)hits[t]);
        return;
    }
    const int64_t BS = (int64_t)gm * DW + gm;
    double *out = part + (b * gridDim.y + blockIdx.y) * BS;
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) {
        const int pi = t + THREADS * k, mm = pi / NQ, q = pi % NQ;
        if (mm < cnt)
#pragma unroll
            for (int c = 0; c < 4; ++c) out[mm * DW + 4 * q + c] = gacc[k][c];
    }
    Ld[t] = lacc;
    __syncthreads();
    if (t < cnt) {
        double s = 0.0;
        for (int r = 0; r < RG; ++r) s += Ld[r * ML + t];
        out[(int64_t)gm * DW + t] = s;
    }
}

// grad_out[m, j] / loss_out[m] = Σ over the chunks of m's problem, in chunk order
__global__ __launch_bounds__(THREADS) void nc_grad_reduce_kernel(Table tb, int d, int gm, int G, const double *__restrict__ part,
                                                                 int64_t M, double *__restrict__ grad_out, double *__restrict__ loss_out)
{
    const int D1 = d + 1, DW = wstride(d);
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= M * (D1 + 1)) return;
    const int64_t m = v / (D1 + 1);
    const int j = (int)(v % (D1 + 1));
    const int p = find_slot(tb.model_start, tb.P + 1, m + tb.model_start[0]);
    if (p >= tb.P) return;                                 // models beyond the table: nothing to sum
    const int64_t lm = m - (tb.model_start[p] - tb.model_start[0]), g = lm / gm, k = lm % gm;
    const int64_t BS = (int64_t)gm * DW + gm, off = j < D1 ? k * DW + j : (int64_t)gm * DW + k;
    double s = 0.0;
    for (int64_t b = tb.block_start[p]; b < tb.block_start[p + 1]; ++b) s += part[(b * G + g) * BS + off];
    if (j < D1) grad_out[m * D1 + j] = s;
    else loss_out[m] = s;
}

// Hessian partials: block (part b of problem p, model lm of p) over the subsample rows [c·chunk, min((c+1)·chunk, nsub)) of p, row i
// of the subsample being entry row_start[p] + i·step.  part[(b·MM + lm)·D1² + j·D1 + k] for j <= k.  Models with a flag are skipped.
template <int MAXB, bool PAIR>
__global__ __launch_bounds__(THREADS) void nc_hess_kernel(Table tb, int d, int MM, int64_t hess_max, int64_t n_emb, const float *__restrict__ E,
                                                          int64_t lde, const float *__restrict__ W, float *__restrict__ part)
{
    extern __shared__ double smd[];
    const int D1 = d + 1, D4 = (D1 + 3) & ~3, nb = D4 / 4, ntri = nb * (nb + 1) / 2;
    float *F = reinterpret_cast<float *>(smd);   // [TE, D4]
    float *Aw = F + TE * D4;                     // [TE]
    const int64_t b = blockIdx.x;
    const int lm = blockIdx.y, t = threadIdx.x;
    const int p = find_slot(tb.block_start, tb.P + 1, b);
    const int64_t parts = tb.block_start[p + 1] - tb.block_start[p], c = b - tb.block_start[p];
    const int64_t ms = tb.model_start[p] - tb.model_start[0], me = tb.model_start[p + 1] - tb.model_start[0];
    if (lm >= me - ms) return;
    const int64_t m = ms + lm;
    if (tb.model_flag[m] != 0) return;
    const int32_t pos = tb.model_pos[m];
    const double w_neg = tb.model_w[2 * m], w_pos = tb.model_w[2 * m + 1];
    const float *w = W + m * D1;
    const int64_t rs = tb.row_start[p], n = tb.row_start[p + 1] - rs;
    const int64_t step = hess_step(n, hess_max), nsub = hess_rows(n, hess_max);
    const int64_t chunk = (nsub + parts - 1) / parts, lo = c * chunk, hi = min(nsub, lo + chunk);

    int bj[MAXB], bk[MAXB];
    float acc[MAXB][16];
    hess_blocks<MAXB, THREADS>(nb, ntri, bj, bk, acc);

    for (int64_t e0 = lo; e0 < hi; e0 += TE) {
        __syncthreads();
        gather_tile<PAIR>(F, D4, d, tb, rs, step, e0, hi, n_emb, E, lde);
        __syncthreads();
        const float zp = hess_row_z(F, D4, D1, w);
        if ((t & 7) == 0) {
            const int64_t i = e0 + (t >> 3);
            Aw[t >> 3] = i < hi ? hess_curvature(tb.y[rs + i * step] == pos ? w_pos : w_neg, zp) : 0.f;
        }
        __syncthreads();
        hess_accumulate<MAXB, TE>(F, D4, Aw, bj, bk, acc);
    }
    hess_store_upper<MAXB>(part + (b * MM + lm) * (int64_t)D1 * D1, D1, bj, bk, acc);
}

// hess[m][j][k] = Σ over the parts of m's problem of part[.][lm][min(j,k)][max(j,k)] in part order (fp64); zero for flagged models
__global__ __launch_bounds__(THREADS) void nc_hess_reduce_kernel(Table tb, int d, int MM, const float *__restrict__ part, int64_t M,
                                                                 double *__restrict__ hess)
{
    const int D1 = d + 1;
    const int64_t per = (int64_t)D1 * D1;
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= M * per) return;
    const int64_t m = v / per;
    const int r = (int)(v % per), j = r / D1, k = r % D1;
    double s = 0.0;
    const int p = find_slot(tb.model_start, tb.P + 1, m + tb.model_start[0]);
    if (p < tb.P && tb.model_flag[m] == 0) {
        const int64_t lm = m - (tb.model_start[p] - tb.model_start[0]);
        const int64_t off = lm * per + (int64_t)min(j, k) * D1 + max(j, k);
        for (int64_t b = tb.block_start[p]; b < tb.block_start[p + 1]; ++b) s += (double)part[b * MM * per + off];
    }
    hess[v] = s;
}

size_t pass_lds(int d, int gm) { return sizeof(double) * THREADS + sizeof(float) * ((size_t)TE * wstride(d) + (size_t)2 * gm * wstride(d) + (size_t)gm * TE); }

}  // namespace

static int check_table(const char *what, int32_t problems, int32_t d, int64_t blocks, const int64_t *row_start, const int64_t *block_start,
                       const int64_t *rows, const int32_t *y, const int32_t *model_start, const int32_t *model_flag, int64_t n_emb,
                       const float *E, int64_t lde, const float *W, int64_t models)
{
    char buf[192];
    if (problems < 1 || d < 1 || blocks < problems || blocks > 0x7fffffffLL || n_emb < 1 || lde < d || models < 0) {
        snprintf(buf, sizeof(buf), "%s: bad sizes (need problems >= 1, blocks >= problems, n_emb >= 1, lde >= d)", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    if (d > MAXD) {
        snprintf(buf, sizeof(buf), "%s: d = %d outside [1, %d]", what, d, MAXD);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (!row_start || !block_start || !rows || !y || !model_start || !model_flag || !E || (models > 0 && !W)) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    return CTGCN_OK;
}

extern "C" int64_t ctgcn_nc_chunks(int64_t n) { return chunks_of(n); }

extern "C" int64_t ctgcn_nc_hess_parts(int64_t n, int64_t hess_max) { return hess_max < 1 ? 0 : hess_parts_of(n, hess_max); }

extern "C" size_t ctgcn_nc_grad_workspace_bytes(int64_t total_chunks, int32_t d, int32_t max_models)
{
    if (total_chunks < 1 || d < 1 || d > MAXD || max_models < 1) return 0;
    const int gm = std::min(max_models, group_max(d));
    const int64_t G = (max_models + gm - 1) / gm;
    return (size_t)total_chunks * G * ((size_t)gm * wstride(d) + gm) * sizeof(double);
}

template <bool PAIR>
static int grad_impl(const char *what, int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *chunk_start,
                     int64_t total_chunks, const int64_t *rows, const int64_t *rows2, const int32_t *y, const int32_t *model_start,
                     const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E, int64_t lde,
                     const float *W, int64_t models, double *loss_out, double *grad_out, void *workspace, size_t workspace_bytes,
                     void *stream)
{
    int rc = check_table(what, problems, d, total_chunks, row_start, chunk_start, rows, y, model_start, model_flag, n_emb, E, lde, W, models);
    if (rc) return rc;
    if (PAIR && !rows2) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (max_models < 1 || max_models > 0xffff * 64) return ctgcn_fail(CTGCN_E_INVALID, what, "bad max_models");
    if (models == 0) return CTGCN_OK;
    if (!model_pos || !model_w || !loss_out || !grad_out || !workspace) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (workspace_bytes < ctgcn_nc_grad_workspace_bytes(total_chunks, d, max_models))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int gm = std::min((int)max_models, group_max(d));
    const int G = (max_models + gm - 1) / gm;
    const Table tb{problems, row_start, chunk_start, rows, rows2, PAIR ? ctgcn_can_vec4(d, E, lde) : 0, y, model_start, model_pos, model_w, model_flag};
    const size_t lds = pass_lds(d, gm);
    if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(nc_pass_kernel<false, PAIR>), lds, "nodecls"))) return rc;
    double *part = (double *)workspace;
    hipLaunchKernelGGL((nc_pass_kernel<false, PAIR>), dim3((unsigned)total_chunks, (unsigned)G), dim3(THREADS), lds, st, tb, (int)d, gm, 0,
                       (const int32_t *)nullptr, n_emb, E, lde, W, models, part, (int32_t *)nullptr, (unsigned long long *)nullptr);
    const int64_t nout = models * (d + 2);
    hipLaunchKernelGGL(nc_grad_reduce_kernel, dim3((unsigned)((nout + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, tb, (int)d, gm, G,
                       (const double *)part, models, grad_out, loss_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_nc_grad_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *chunk_start,
                                 int64_t total_chunks, const int64_t *rows, const int32_t *y, const int32_t *model_start,
                                 const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E,
                                 int64_t lde, const float *W, int64_t models, double *loss_out, double *grad_out, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return grad_impl<false>("nc_grad", problems, d, max_models, row_start, chunk_start, total_chunks, rows, nullptr, y, model_start, model_pos,
                            model_w, model_flag, n_emb, E, lde, W, models, loss_out, grad_out, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_ec_grad_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *chunk_start,
                                 int64_t total_chunks, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                                 const int32_t *model_start, const int32_t *model_pos, const double *model_w, const int32_t *model_flag,
                                 int64_t n_emb, const float *E, int64_t lde, const float *W, int64_t models, double *loss_out,
                                 double *grad_out, void *workspace, size_t workspace_bytes, void *stream)
{
    return grad_impl<true>("ec_grad", problems, d, max_models, row_start, chunk_start, total_chunks, rows, rows2, y, model_start, model_pos,
                           model_w, model_flag, n_emb, E, lde, W, models, loss_out, grad_out, workspace, workspace_bytes, stream);
}

extern "C" size_t ctgcn_nc_hess_workspace_bytes(int64_t total_parts, int32_t d, int32_t max_models)
{
    if (total_parts < 1 || d < 1 || d > MAXD || max_models < 1) return 0;
    return (size_t)total_parts * max_models * (size_t)(d + 1) * (d + 1) * sizeof(float);
}

template <bool PAIR>
static int hess_impl(const char *what, int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *part_start,
                     int64_t total_parts, int64_t hess_max, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                     const int32_t *model_start, const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb,
                     const float *E, int64_t lde, const float *W, int64_t models, double *hess_out, void *workspace, size_t workspace_bytes,
                     void *stream)
{
    int rc = check_table(what, problems, d, total_parts, row_start, part_start, rows, y, model_start, model_flag, n_emb, E, lde, W, models);
    if (rc) return rc;
    if (PAIR && !rows2) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (max_models < 1 || max_models > 0xffff || hess_max < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "bad max_models or hess_max");
    if (models == 0) return CTGCN_OK;
    if (!model_pos || !model_w || !hess_out || !workspace) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (workspace_bytes < ctgcn_nc_hess_workspace_bytes(total_parts, d, max_models))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const Table tb{problems, row_start, part_start, rows, rows2, PAIR ? ctgcn_can_vec4(d, E, lde) : 0, y, model_start, model_pos, model_w, model_flag};
    const int D1 = d + 1, D4 = (D1 + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)TE * D4 + TE);
    float *part = (float *)workspace;
    if (d <= 128)        // (d+1) padded to 4: at most 33 column blocks, 561 upper-triangle tiles -> 3 per thread
        hipLaunchKernelGGL((nc_hess_kernel<3, PAIR>), dim3((unsigned)total_parts, (unsigned)max_models), dim3(THREADS), lds, st, tb, (int)d,
                           (int)max_models, hess_max, n_emb, E, lde, W, part);
    else                 // at most 65 column blocks, 2145 tiles -> 9 per thread
        hipLaunchKernelGGL((nc_hess_kernel<9, PAIR>), dim3((unsigned)total_parts, (unsigned)max_models), dim3(THREADS), lds, st, tb, (int)d,
                           (int)max_models, hess_max, n_emb, E, lde, W, part);
    const int64_t total = models * D1 * D1;
    hipLaunchKernelGGL(nc_hess_reduce_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, tb, (int)d,
                       (int)max_models, (const float *)part, models, hess_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_nc_hess_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *part_start,
                                 int64_t total_parts, int64_t hess_max, const int64_t *rows, const int32_t *y, const int32_t *model_start,
                                 const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E,
                                 int64_t lde, const float *W, int64_t models, double *hess_out, void *workspace, size_t workspace_bytes,
                                 void *stream)
{
    return hess_impl<false>("nc_hess", problems, d, max_models, row_start, part_start, total_parts, hess_max, rows, nullptr, y, model_start,
                            model_pos, model_w, model_flag, n_emb, E, lde, W, models, hess_out, workspace, workspace_bytes, stream);
}

extern "C" int ctgcn_ec_hess_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *part_start,
                                 int64_t total_parts, int64_t hess_max, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                                 const int32_t *model_start, const int32_t *model_pos, const double *model_w, const int32_t *model_flag,
                                 int64_t n_emb, const float *E, int64_t lde, const float *W, int64_t models, double *hess_out,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    return hess_impl<true>("ec_hess", problems, d, max_models, row_start, part_start, total_parts, hess_max, rows, rows2, y, model_start,
                           model_pos, model_w, model_flag, n_emb, E, lde, W, models, hess_out, workspace, workspace_bytes, stream);
}

template <bool PAIR>
static int predict_impl(const char *what, int32_t problems, int32_t d, int32_t max_classes, int32_t groups, const int64_t *row_start,
                        const int64_t *chunk_start, int64_t total_chunks, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                        const int32_t *n_classes, const int32_t *model_start, const int32_t *model_flag, int64_t n_emb, const float *E,
                        int64_t lde, const float *W, int64_t models, int32_t *pred_out, int64_t *correct_out, void *stream)
{
    int rc = check_table(what, problems, d, total_chunks, row_start, chunk_start, rows, y, model_start, model_flag, n_emb, E, lde, W, models);
    if (rc) return rc;
    if (PAIR && !rows2) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (groups < 1 || max_classes < 2) return ctgcn_fail(CTGCN_E_INVALID, what, "need groups >= 1 and max_classes >= 2");
    if (max_classes > group_max(d)) {
        char buf[96];
        snprintf(buf, sizeof(buf), "%d classes, at most %d at d = %d (the models of one block)", (int)max_classes, group_max(d), (int)d);
        return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, buf);
    }
    if (!n_classes || !pred_out || !correct_out) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    CTGCN_TRY(hipMemsetAsync(correct_out, 0, sizeof(int64_t) * problems * groups, st));
    if (models == 0) return CTGCN_OK;
    const int mpg = max_classes == 2 ? 1 : max_classes;
    const int gm = std::min(group_max(d), groups * mpg);
    const int gpb = gm / mpg;
    const int G = (groups + gpb - 1) / gpb;
    if (G > 0xffff) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "too many C groups");
    const Table tb{problems, row_start, chunk_start, rows, rows2, PAIR ? ctgcn_can_vec4(d, E, lde) : 0, y, model_start, nullptr, nullptr, model_flag};
    const size_t lds = pass_lds(d, gm);
    if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(nc_pass_kernel<true, PAIR>), lds, "nodecls"))) return rc;
    hipLaunchKernelGGL((nc_pass_kernel<true, PAIR>), dim3((unsigned)total_chunks, (unsigned)G), dim3(THREADS), lds, st, tb, (int)d, gm,
                       (int)groups, n_classes, n_emb, E, lde, W, models, (double *)nullptr, pred_out, (unsigned long long *)correct_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_nc_predict_f32(int32_t problems, int32_t d, int32_t max_classes, int32_t groups, const int64_t *row_start,
                                    const int64_t *chunk_start, int64_t total_chunks, const int64_t *rows, const int32_t *y,
                                    const int32_t *n_classes, const int32_t *model_start, const int32_t *model_flag, int64_t n_emb,
                                    const float *E, int64_t lde, const float *W, int64_t models, int32_t *pred_out, int64_t *correct_out,
                                    void *stream)
{
    return predict_impl<false>("nc_predict", problems, d, max_classes, groups, row_start, chunk_start, total_chunks, rows, nullptr, y, n_classes,
                               model_start, model_flag, n_emb, E, lde, W, models, pred_out, correct_out, stream);
}

extern "C" int ctgcn_ec_predict_f32(int32_t problems, int32_t d, int32_t max_classes, int32_t groups, const int64_t *row_start,
                                    const int64_t *chunk_start, int64_t total_chunks, const int64_t *rows, const int64_t *rows2,
                                    const int32_t *y, const int32_t *n_classes, const int32_t *model_start, const int32_t *model_flag,
                                    int64_t n_emb, const float *E, int64_t lde, const float *W, int64_t models, int32_t *pred_out,
                                    int64_t *correct_out, void *stream)
{
    return predict_impl<true>("ec_predict", problems, d, max_classes, groups, row_start, chunk_start, total_chunks, rows, rows2, y, n_classes,
                              model_start, model_flag, n_emb, E, lde, W, models, pred_out, correct_out, stream);
}
