// ctgcn_supervised.hip — classifier head of the supervised trainer (reference models.py:46-125, metrics.py:169-209) on the GPU.
//
// An item is a labelled node a (NODE) or a labelled pair (a, b) (HADAMARD, DOT); its feature is f = E[a], f = E[a] ⊙ E[b], or the
// score z = <E[a], E[b]> with no head behind it (DOT).  Three passes:
//   - head forward: out[i, c] = act(W[c]·f_i + bias[c]).  A tile of 32 features is formed in LDS while it is staged (the pair gather of
//     ctgcn_nodecls.hip), so no [items, d] array exists.  DOT: one wave per item.
//   - loss pass over the logits: cross entropy (or BCE with logits for DOT), its mean, the count of correct predictions, the
//     probabilities and dlogits = (p - onehot) / items, times SELU' when the head has the activation.
//   - head backward in pull form: the caller gives the incidence CSR node -> (item, other endpoint), cut into pieces of at most PIECE
//     incidences; a wave owns a piece, sums it in CSR order and writes the dE row (or, for a node of several pieces, a partial row that
//     a second kernel adds in piece order).  Nodes with no incidence are pieces of length 0: their rows are written as zeros.
//     dW and db come from a tile pass like the forward's, per-block fp64 partials summed in block order.
// No float atomics anywhere: block and piece counts are functions of the sizes alone, so repeated calls are bit-identical.
// All sums run in fp64 (the kernels are gather-bound; the fp64 FMAs are free beside the row loads) and are rounded to fp32 once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ctgcn_logreg.h"
#include "ctgcn_try.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TE = 32;                 // items per tile
constexpr int MAXD = 256;
constexpr int MAXC = 32;
constexpr int PIECE = 512;             // incidences per pull piece
constexpr int MAX_PART_BLOCKS = 1024;  // blocks of the loss pass and of the dW pass
constexpr int MAX_GRID = 2048;         // grid-stride cap of the forward and pull kernels
constexpr int TILES_PER_DW_BLOCK = 4;
constexpr int PAIRS = 9;               // (class, column quad) pairs per thread of the dW pass: 32 x 65 <= 9 x 256
constexpr double SELU_ALPHA = 1.6732632423543772848170429916717;
constexpr double SELU_SCALE = 1.0507009873554804934193349852946;

enum { NODE = CTGCN_CLS_NODE, HADAMARD = CTGCN_CLS_HADAMARD, DOT = CTGCN_CLS_DOT };

// LDS row stride of tiles and weights: d rounded up to 4, with an odd number of 16-byte slots (see ctgcn_nodecls.hip)
__host__ __device__ __forceinline__ int wstride(int d)
{
    int w = (d + 3) & ~3;
    if (((w >> 2) & 1) == 0) w += 4;
    return w;
}
__host__ __device__ __forceinline__ int64_t loss_blocks(int64_t items)
{
    const int64_t c = (items + THREADS - 1) / THREADS;
    return c < 1 ? 1 : (c < MAX_PART_BLOCKS ? c : MAX_PART_BLOCKS);
}
__host__ __device__ __forceinline__ int64_t dw_blocks(int64_t items)
{
    const int64_t c = (items + (int64_t)TILES_PER_DW_BLOCK * TE - 1) / ((int64_t)TILES_PER_DW_BLOCK * TE);
    return c < 1 ? 1 : (c < MAX_PART_BLOCKS ? c : MAX_PART_BLOCKS);
}

// X [TE, DW]: row r = the feature of item i0 + r (zero past `items`, zero for an index outside [0, n_nodes)), zero in columns >= d.
// vec4: half a wave per row and a float4 per lane, the loads of a wave's 8 rows issued before the first LDS write.
template <int MODE>
__device__ __forceinline__ void stage_tile(float *X, int DW, int d, int vec4, const int64_t *__restrict__ a, const int64_t *__restrict__ b,
                                           int64_t i0, int64_t items, int64_t n_nodes, const float *__restrict__ E, int64_t lde)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (vec4) {
        constexpr int RW = TE / WAVES / 2;                 // rows per half wave
        const int half = lane >> 5, hl = lane & 31, NQ = DW >> 2, dq = d >> 2;
        int64_t ia[RW], ib[RW];
        bool valid[RW];
#pragma unroll
        for (int k = 0; k < RW; ++k) {                     // unconditional loads: an item past the end reads item i0 and is dropped
            const int64_t i = i0 + wave * (2 * RW) + 2 * k + half;
            const bool ok = i < items;
            const int64_t e = ok ? i : i0;
            ia[k] = a[e];
            ib[k] = MODE == NODE ? 0 : b[e];
            valid[k] = ok && ia[k] >= 0 && ia[k] < n_nodes && ib[k] >= 0 && ib[k] < n_nodes;
            ia[k] = valid[k] ? ia[k] : 0;
            ib[k] = valid[k] ? ib[k] : 0;
        }
        for (int q = hl; q < NQ; q += 32) {
            const int qs = q < dq ? q : 0;                 // padding quads read quad 0 and store zeros
            float4 va[RW], vb[RW];
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                va[k] = *reinterpret_cast<const float4 *>(E + ia[k] * lde + 4 * qs);
                if (MODE != NODE) vb[k] = *reinterpret_cast<const float4 *>(E + ib[k] * lde + 4 * qs);
            }
#pragma unroll
            for (int k = 0; k < RW; ++k) {
                float4 o = va[k];
                if (MODE != NODE) o = make_float4(va[k].x * vb[k].x, va[k].y * vb[k].y, va[k].z * vb[k].z, va[k].w * vb[k].w);
                if (!valid[k] || q >= dq) o = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(X + (wave * (2 * RW) + 2 * k + half) * DW + 4 * q) = o;
            }
        }
        return;
    }
    for (int r = wave; r < TE; r += WAVES) {
        const int64_t i = i0 + r;
        const bool ok = i < items;
        const int64_t na = ok ? a[i] : -1;
        const int64_t nb = MODE == NODE ? 0 : (ok ? b[i] : -1);
        const bool valid = na >= 0 && na < n_nodes && nb >= 0 && nb < n_nodes;
        float *out = X + r * DW;
        for (int c = lane; c < DW; c += 64) {
            float v = 0.f;
            if (valid && c < d) v = MODE == NODE ? E[na * lde + c] : E[na * lde + c] * E[nb * lde + c];
            out[c] = v;
        }
    }
}

__device__ __forceinline__ double selu(double x) { return SELU_SCALE * (x > 0.0 ? x : SELU_ALPHA * expm1(x)); }
// dSELU/dx from y = SELU(x): scale for x > 0, scale·alpha·e^x = y + scale·alpha otherwise (x = 0 takes that branch, as torch does)
__device__ __forceinline__ double selu_grad_from_out(double y) { return y > 0.0 ? SELU_SCALE : y + SELU_SCALE * SELU_ALPHA; }

// out[i, c] = act(W[c]·f_i + bias[c]).  Thread (row r = t % 32, class lane cg = t / 32) owns classes cg, cg + 8, cg + 16, cg + 24.
template <int MODE>
__global__ __launch_bounds__(THREADS) void cls_fwd_kernel(int d, int C, int act, int vec4, int64_t items, const int64_t *__restrict__ a,
                                                          const int64_t *__restrict__ b, int64_t n_nodes, const float *__restrict__ E,
                                                          int64_t lde, const float *__restrict__ W, const float *__restrict__ bias,
                                                          float *__restrict__ out)
{
    extern __shared__ __align__(16) float sm[];
    const int DW = wstride(d), NQ = DW >> 2, t = threadIdx.x;
    float *X = sm;                    // [TE, DW]
    float *Wl = X + TE * DW;          // [C, DW]
    for (int i = t; i < C * DW; i += THREADS) {
        const int c = i / DW, col = i % DW;
        Wl[i] = col < d ? W[(int64_t)c * d + col] : 0.f;
    }
    const int r = t & 31, cg = t >> 5;
    const int64_t ntiles = (items + TE - 1) / TE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * TE;
        __syncthreads();                                   // the previous tile is done with X (first pass: Wl written)
        stage_tile<MODE>(X, DW, d, vec4, a, b, i0, items, n_nodes, E, lde);
        __syncthreads();
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int q = 0; q < NQ; ++q) {
            const float4 x = *reinterpret_cast<const float4 *>(X + r * DW + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = cg + 8 * k;
                if (c < C) {
                    const float4 w = *reinterpret_cast<const float4 *>(Wl + c * DW + 4 * q);
                    acc[k] = fma((double)x.x, (double)w.x, acc[k]);
                    acc[k] = fma((double)x.y, (double)w.y, acc[k]);
                    acc[k] = fma((double)x.z, (double)w.z, acc[k]);
                    acc[k] = fma((double)x.w, (double)w.w, acc[k]);
                }
            }
        }
        const int64_t i = i0 + r;
        if (i < items)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = cg + 8 * k;
                if (c < C) {
                    double z = acc[k] + (bias ? (double)bias[c] : 0.0);
                    if (act) z = selu(z);
                    out[i * C + c] = (float)z;
                }
            }
    }
}

// z[i] = <E[a_i], E[b_i]>: a wave per item, fixed-order butterfly
__global__ __launch_bounds__(THREADS) void cls_dot_fwd_kernel(int d, int64_t items, const int64_t *__restrict__ a, const int64_t *__restrict__ b,
                                                              int64_t n_nodes, const float *__restrict__ E, int64_t lde, float *__restrict__ z)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * WAVES + wave; i < items; i += (int64_t)gridDim.x * WAVES) {
        const int64_t na = a[i], nb = b[i];
        const bool valid = na >= 0 && na < n_nodes && nb >= 0 && nb < n_nodes;
        double s = 0.0;
        if (valid)
            for (int c = lane; c < d; c += 64) s = fma((double)E[na * lde + c], (double)E[nb * lde + c], s);
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) z[i] = (float)s;
    }
}

// Loss pass.  Thread t of block b walks items (b + j·blocks)·THREADS + t; part_loss[b] / part_correct[b] are the block's sums.
__global__ __launch_bounds__(THREADS) void cls_loss_kernel(int dot, int act, int C, int64_t items, const float *__restrict__ logits,
                                                           const int64_t *__restrict__ labels, float *__restrict__ prob,
                                                           float *__restrict__ dl, double *__restrict__ part_loss,
                                                           int64_t *__restrict__ part_correct)
{
    __shared__ double ls[THREADS];
    __shared__ int lc[THREADS];
    const int t = threadIdx.x;
    const double inv = 1.0 / (double)items;
    double loss = 0.0;
    int correct = 0;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + t; i < items; i += (int64_t)gridDim.x * THREADS) {
        const int64_t y = labels[i];
        if (dot) {
            const double z = (double)logits[i], p = sigmoid(z);
            const bool yv = y == 1;
            loss += softplus(yv ? -z : z);
            correct += ((z > 0.0) == yv) && (y == 0 || y == 1);
            if (prob) prob[i] = (float)p;
            if (dl) dl[i] = (float)((p - (yv ? 1.0 : 0.0)) * inv);
            continue;
        }
        const float *row = logits + i * C;
        float m = row[0];
        int best = 0;
        for (int c = 1; c < C; ++c) {
            const float v = row[c];
            if (v > m) { m = v; best = c; }                // the first maximal class wins ties
        }
        double se = 0.0;
        for (int c = 0; c < C; ++c) se += exp((double)row[c] - (double)m);
        const double lse = (double)m + log(se);
        const bool yok = y >= 0 && y < C;
        loss += lse - (yok ? (double)row[y] : 0.0);
        correct += yok && best == (int)y;
        for (int c = 0; c < C; ++c) {
            const double zc = (double)row[c], p = exp(zc - lse);
            if (prob) prob[i * C + c] = (float)p;
            if (dl) {
                double g = (p - (c == y ? 1.0 : 0.0)) * inv;
                if (act) g *= selu_grad_from_out(zc);
                dl[i * C + c] = (float)g;
            }
        }
    }
    ls[t] = loss;
    lc[t] = correct;
    __syncthreads();
    for (int s = THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            ls[t] += ls[t + s];
            lc[t] += lc[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        part_loss[blockIdx.x] = ls[0];
        part_correct[blockIdx.x] = lc[0];
    }
}

__global__ void cls_loss_finish_kernel(int64_t blocks, int64_t items, const double *__restrict__ part_loss,
                                       const int64_t *__restrict__ part_correct, double *__restrict__ loss_out, int64_t *__restrict__ correct_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    int64_t c = 0;
    for (int64_t b = 0; b < blocks; ++b) {
        s += part_loss[b];
        c += part_correct[b];
    }
    loss_out[0] = s / (double)items;
    correct_out[0] = c;
}

// dW / db partials: part[blk·(C·DW + C) ...] = Σ over the block's tiles of dl[i, c]·f_i ([C, DW]) then Σ dl[i, c] ([C]).
template <int MODE>
__global__ __launch_bounds__(THREADS) void cls_dw_kernel(int d, int C, int vec4, int64_t items, const int64_t *__restrict__ a,
                                                         const int64_t *__restrict__ b, int64_t n_nodes, const float *__restrict__ E,
                                                         int64_t lde, const float *__restrict__ dl, double *__restrict__ part)
{
    extern __shared__ __align__(16) float sm[];
    const int DW = wstride(d), NQ = DW >> 2, t = threadIdx.x;
    float *X = sm;                    // [TE, DW]
    float *R = X + TE * DW;           // [TE, C]
    double g[PAIRS][4];
#pragma unroll
    for (int k = 0; k < PAIRS; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) g[k][c] = 0.0;
    double gb = 0.0;
    const int64_t ntiles = (items + TE - 1) / TE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * TE;
        __syncthreads();
        stage_tile<MODE>(X, DW, d, vec4, a, b, i0, items, n_nodes, E, lde);
        for (int u = t; u < TE * C; u += THREADS) {
            const int64_t i = i0 + u / C;
            R[u] = i < items ? dl[i * C + u % C] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) {
            const int pi = t + THREADS * k, cc = pi / NQ, q = pi % NQ;
            if (cc < C)
                for (int r = 0; r < TE; ++r) {
                    const double rv = (double)R[r * C + cc];
                    const float4 x = *reinterpret_cast<const float4 *>(X + r * DW + 4 * q);
                    g[k][0] = fma(rv, (double)x.x, g[k][0]);
                    g[k][1] = fma(rv, (double)x.y, g[k][1]);
                    g[k][2] = fma(rv, (double)x.z, g[k][2]);
                    g[k][3] = fma(rv, (double)x.w, g[k][3]);
                }
        }
        if (t < C)
            for (int r = 0; r < TE; ++r) gb += (double)R[r * C + t];
    }
    double *out = part + (int64_t)blockIdx.x * ((int64_t)C * DW + C);
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) {
        const int pi = t + THREADS * k, cc = pi / NQ, q = pi % NQ;
        if (cc < C)
#pragma unroll
            for (int c = 0; c < 4; ++c) out[cc * DW + 4 * q + c] = g[k][c];
    }
    if (t < C) out[(int64_t)C * DW + t] = gb;
}

// dW[c, col] / db[c] = Σ over the blocks in block order
__global__ __launch_bounds__(THREADS) void cls_dw_reduce_kernel(int d, int C, int64_t blocks, const double *__restrict__ part,
                                                                float *__restrict__ dW, float *__restrict__ db)
{
    const int DW = wstride(d);
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (v >= (int64_t)C * d + C) return;
    const int64_t BS = (int64_t)C * DW + C;
    const bool isb = v >= (int64_t)C * d;
    const int64_t off = isb ? (int64_t)C * DW + (v - (int64_t)C * d) : (v / d) * DW + v % d;
    double s = 0.0;
    for (int64_t k = 0; k < blocks; ++k) s += part[k * BS + off];
    if (!isb) dW[v] = (float)s;
    else if (db) db[v - (int64_t)C * d] = (float)s;
}

// Pull backward: a wave per piece [piece_ptr[p], piece_ptr[p+1]) of node piece_node[p]'s incidences, summed in CSR order.  The row goes to
// dE when piece_slot[p] < 0, else to row piece_slot[p] of hub_part (fp64).  Lane l owns columns l, l + 64, l + 128, l + 192.
template <int MODE>
__global__ __launch_bounds__(THREADS) void cls_pull_kernel(int d, int C, int64_t items, int64_t n_nodes, int64_t n_pieces,
                                                           const int64_t *__restrict__ piece_ptr, const int64_t *__restrict__ piece_node,
                                                           const int64_t *__restrict__ piece_slot, const int64_t *__restrict__ inc_item,
                                                           const int64_t *__restrict__ inc_other, const float *__restrict__ E, int64_t lde,
                                                           const float *__restrict__ W, const float *__restrict__ dl, float *__restrict__ dE,
                                                           int64_t ldde, double *__restrict__ hub_part)
{
    extern __shared__ __align__(16) float sm[];
    float *Wl = sm;                   // [C, d] (NODE, HADAMARD)
    if (MODE != DOT) {
        for (int i = threadIdx.x; i < C * d; i += THREADS) Wl[i] = W[i];
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t p = (int64_t)blockIdx.x * WAVES + wave; p < n_pieces; p += (int64_t)gridDim.x * WAVES) {
        const int64_t lo = piece_ptr[p], hi = piece_ptr[p + 1], v = piece_node[p], slot = piece_slot[p];
        if (v < 0 || v >= n_nodes) continue;               // wave-uniform
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (MODE == NODE) {
            double s = 0.0;                                // lane c: Σ dl[item, c]
            for (int64_t j = lo; j < hi; ++j) {
                const int64_t it = inc_item[j];
                if (it >= 0 && it < items && lane < C) s += (double)dl[it * C + lane];
            }
            for (int c = 0; c < C; ++c) {
                const double sc = __shfl(s, c, 64);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int col = lane + 64 * k;
                    if (col < d) acc[k] = fma(sc, (double)Wl[c * d + col], acc[k]);
                }
            }
        } else {
            // one incidence per trip: with several rows of a wave in flight (4 per trip, loads issued first) the head measured 11-17 % slower
            // on config 5's last snapshot (8 M pairs): the 8 waves per SIMD already keep enough rows in flight
            for (int64_t j = lo; j < hi; ++j) {
                const int64_t it = inc_item[j], ot = inc_other[j];
                if (it < 0 || it >= items || ot < 0 || ot >= n_nodes) continue;      // wave-uniform
                const float *er = E + ot * lde;
                float e[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int col = lane + 64 * k;
                    e[k] = col < d ? er[col] : 0.f;
                }
                if (MODE == DOT) {
                    const double gi = (double)dl[it];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fma(gi, (double)e[k], acc[k]);
                } else {
                    double tt[4] = {0.0, 0.0, 0.0, 0.0};
                    for (int c = 0; c < C; ++c) {
                        const double gc = (double)dl[it * C + c];                    // wave-uniform address
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int col = lane + 64 * k;
                            if (col < d) tt[k] = fma(gc, (double)Wl[c * d + col], tt[k]);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fma(tt[k], (double)e[k], acc[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            if (col < d) {
                if (slot < 0) dE[v * ldde + col] = (float)acc[k];
                else hub_part[slot * d + col] = acc[k];
            }
        }
    }
}

// dE[hub_node[h]] = Σ of its partial rows [hub_slot_ptr[h], hub_slot_ptr[h+1]) in piece order
__global__ __launch_bounds__(THREADS) void cls_hub_sum_kernel(int d, int64_t n_hubs, int64_t n_nodes, const int64_t *__restrict__ hub_node,
                                                              const int64_t *__restrict__ hub_slot_ptr, const double *__restrict__ hub_part,
                                                              float *__restrict__ dE, int64_t ldde)
{
    const int64_t u = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (u >= n_hubs * d) return;
    const int64_t h = u / d, v = hub_node[h];
    const int col = (int)(u % d);
    if (v < 0 || v >= n_nodes) return;
    double s = 0.0;
    for (int64_t k = hub_slot_ptr[h]; k < hub_slot_ptr[h + 1]; ++k) s += hub_part[k * d + col];
    dE[v * ldde + col] = (float)s;
}

// sizes shared by the three entry points: mode, d, and n_class for the modes with a head
int check_sizes(const char *what, int32_t mode, int64_t items, int32_t d, int32_t n_class)
{
    char buf[192];
    if (mode != NODE && mode != HADAMARD && mode != DOT) return ctgcn_fail(CTGCN_E_INVALID, what, "mode must be CTGCN_CLS_NODE, _HADAMARD or _DOT");
    if (items < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need items >= 1");
    if (d < 1 || d > MAXD) {
        snprintf(buf, sizeof(buf), "%s: d = %d outside [1, %d]", what, d, MAXD);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (mode != DOT && (n_class < 2 || n_class > MAXC)) {
        snprintf(buf, sizeof(buf), "%s: n_class = %d outside [2, %d]", what, n_class, MAXC);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    return CTGCN_OK;
}

unsigned grid_of(int64_t work) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(work, MAX_GRID)); }

}  // namespace

extern "C" int64_t ctgcn_cls_pull_piece(void) { return PIECE; }

extern "C" int ctgcn_cls_check_items(int32_t mode, int64_t items, const int64_t *a, const int64_t *b, int64_t n_nodes, void *stream)
{
    const char *what = "cls_check_items";
    if (mode != NODE && mode != HADAMARD && mode != DOT) return ctgcn_fail(CTGCN_E_INVALID, what, "mode must be CTGCN_CLS_NODE, _HADAMARD or _DOT");
    if (items < 0 || n_nodes < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need items >= 0 and n_nodes >= 1");
    if (items == 0) return CTGCN_OK;
    if (!a || (mode != NODE && !b)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> host((size_t)items);
    for (const int64_t *src : {a, mode != NODE ? b : (const int64_t *)nullptr}) {
        if (!src) continue;
        CTGCN_TRY(hipMemcpyAsync(host.data(), src, sizeof(int64_t) * (size_t)items, hipMemcpyDeviceToHost, st));
        CTGCN_TRY(hipStreamSynchronize(st));
        for (int64_t i = 0; i < items; ++i)
            if (host[i] < 0 || host[i] >= n_nodes) {
                char buf[160];
                snprintf(buf, sizeof(buf), "%s: item %lld has node index %lld outside [0, %lld)", what, (long long)i, (long long)host[i],
                         (long long)n_nodes);
                return ctgcn_set_error_(CTGCN_E_INVALID, buf);
            }
    }
    return CTGCN_OK;
}

extern "C" int ctgcn_cls_head_fwd_f32(int32_t mode, int32_t act, int64_t items, int32_t d, int32_t n_class, const int64_t *a, const int64_t *b,
                                      int64_t n_nodes, const float *E, int64_t lde, const float *W, const float *bias, float *out, void *stream)
{
    const char *what = "cls_head_fwd";
    int rc = check_sizes(what, mode, items, d, n_class);
    if (rc) return rc;
    if (n_nodes < 1 || lde < d) return ctgcn_fail(CTGCN_E_INVALID, what, "need n_nodes >= 1 and lde >= d");
    if (act != 0 && act != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (SELU)");
    if (!a || (mode != NODE && !b) || !E || !out || (mode != DOT && !W)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (mode == DOT) {
        hipLaunchKernelGGL(cls_dot_fwd_kernel, dim3(grid_of((items + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, (int)d, items, a, b, n_nodes, E,
                           lde, out);
        CTGCN_TRY(hipGetLastError());
        return CTGCN_OK;
    }
    const int DW = wstride(d), vec4 = ctgcn_can_vec4(d, E, lde);
    const size_t lds = sizeof(float) * ((size_t)TE * DW + (size_t)n_class * DW);
    const dim3 grid(grid_of((items + TE - 1) / TE));
    if (mode == NODE) {
        if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(cls_fwd_kernel<NODE>), lds, what))) return rc;
        hipLaunchKernelGGL(cls_fwd_kernel<NODE>, grid, dim3(THREADS), lds, st, (int)d, (int)n_class, (int)act, vec4, items, a, b, n_nodes, E, lde,
                           W, bias, out);
    } else {
        if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(cls_fwd_kernel<HADAMARD>), lds, what))) return rc;
        hipLaunchKernelGGL(cls_fwd_kernel<HADAMARD>, grid, dim3(THREADS), lds, st, (int)d, (int)n_class, (int)act, vec4, items, a, b, n_nodes, E,
                           lde, W, bias, out);
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_cls_loss_workspace_bytes(int64_t items)
{
    if (items < 1) return 0;
    return (size_t)loss_blocks(items) * (sizeof(double) + sizeof(int64_t));
}

extern "C" int ctgcn_cls_loss_f32(int32_t mode, int32_t act, int64_t items, int32_t n_class, const float *logits, const int64_t *labels,
                                  double *loss_out, int64_t *correct_out, float *prob, float *dlogits, void *workspace, size_t workspace_bytes,
                                  void *stream)
{
    const char *what = "cls_loss";
    int rc = check_sizes(what, mode, items, 1, n_class);
    if (rc) return rc;
    if (act != 0 && act != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (SELU)");
    if (!logits || !labels || !loss_out || !correct_out || !workspace) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (workspace_bytes < ctgcn_cls_loss_workspace_bytes(items)) return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = loss_blocks(items);
    double *part_loss = (double *)workspace;
    int64_t *part_correct = (int64_t *)(part_loss + blocks);
    hipLaunchKernelGGL(cls_loss_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, mode == DOT ? 1 : 0, mode == DOT ? 0 : (int)act,
                       (int)n_class, items, logits, labels, prob, dlogits, part_loss, part_correct);
    hipLaunchKernelGGL(cls_loss_finish_kernel, dim3(1), dim3(64), 0, st, blocks, items, (const double *)part_loss,
                       (const int64_t *)part_correct, loss_out, correct_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_cls_head_bwd_workspace_bytes(int64_t items, int32_t d, int32_t n_class, int64_t hub_pieces)
{
    if (items < 1 || d < 1 || d > MAXD || n_class < 1 || n_class > MAXC || hub_pieces < 0) return 0;
    return sizeof(double) * ((size_t)hub_pieces * d + (size_t)dw_blocks(items) * ((size_t)n_class * wstride(d) + n_class)) + 16;
}

extern "C" int ctgcn_cls_head_bwd_f32(int32_t mode, int64_t items, int32_t d, int32_t n_class, const int64_t *a, const int64_t *b,
                                      int64_t n_nodes, const float *E, int64_t lde, const float *W, const float *dlogits, int64_t n_pieces,
                                      const int64_t *piece_ptr, const int64_t *piece_node, const int64_t *piece_slot, const int64_t *inc_item,
                                      const int64_t *inc_other, int64_t n_hubs, const int64_t *hub_node, const int64_t *hub_slot_ptr,
                                      int64_t hub_pieces, float *dE, int64_t ldde, float *dW, float *db, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const char *what = "cls_head_bwd";
    int rc = check_sizes(what, mode, items, d, n_class);
    if (rc) return rc;
    const int C = mode == DOT ? 1 : n_class;
    if (n_nodes < 1 || lde < d) return ctgcn_fail(CTGCN_E_INVALID, what, "need n_nodes >= 1 and lde >= d");
    if (!a || (mode != NODE && !b) || !E || !dlogits || (mode != DOT && !W) || !workspace) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (mode == DOT && (dW || db)) return ctgcn_fail(CTGCN_E_INVALID, what, "CTGCN_CLS_DOT has no head: dW and db must be null");
    if (db && !dW) return ctgcn_fail(CTGCN_E_INVALID, what, "db needs dW");
    if (workspace_bytes < ctgcn_cls_head_bwd_workspace_bytes(items, d, C, hub_pieces)) return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double *hub_part = (double *)workspace;
    double *dw_part = hub_part + (size_t)hub_pieces * d;
    if (dE) {
        if (n_pieces < n_nodes || n_hubs < 0 || hub_pieces < 0 || ldde < d) return ctgcn_fail(CTGCN_E_INVALID, what, "bad piece table sizes or ldde < d");
        if (!piece_ptr || !piece_node || !piece_slot || !inc_item || (mode != NODE && !inc_other) || (n_hubs > 0 && (!hub_node || !hub_slot_ptr)))
            return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
        const size_t lds = mode == DOT ? 0 : sizeof(float) * (size_t)C * d;
        const dim3 grid(grid_of((n_pieces + WAVES - 1) / WAVES));
#define CTGCN_CLS_PULL(M)                                                                                                                       \
    hipLaunchKernelGGL(cls_pull_kernel<M>, grid, dim3(THREADS), lds, st, (int)d, C, items, n_nodes, n_pieces, piece_ptr, piece_node, piece_slot, \
                       inc_item, inc_other, E, lde, W, dlogits, dE, ldde, hub_part)
        if (mode == NODE) CTGCN_CLS_PULL(NODE);
        else if (mode == HADAMARD) CTGCN_CLS_PULL(HADAMARD);
        else CTGCN_CLS_PULL(DOT);
#undef CTGCN_CLS_PULL
        if (n_hubs > 0)
            hipLaunchKernelGGL(cls_hub_sum_kernel, dim3((unsigned)((n_hubs * d + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (int)d, n_hubs,
                               n_nodes, hub_node, hub_slot_ptr, (const double *)hub_part, dE, ldde);
    }
    if (dW) {
        const int DW = wstride(d), vec4 = ctgcn_can_vec4(d, E, lde);
        const int64_t blocks = dw_blocks(items);
        const size_t lds = sizeof(float) * ((size_t)TE * DW + (size_t)TE * C);
        if (mode == NODE) {
            if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(cls_dw_kernel<NODE>), lds, what))) return rc;
            hipLaunchKernelGGL(cls_dw_kernel<NODE>, dim3((unsigned)blocks), dim3(THREADS), lds, st, (int)d, C, vec4, items, a, b, n_nodes, E, lde,
                               dlogits, dw_part);
        } else {
            if ((rc = ctgcn_opt_in_lds(reinterpret_cast<const void *>(cls_dw_kernel<HADAMARD>), lds, what))) return rc;
            hipLaunchKernelGGL(cls_dw_kernel<HADAMARD>, dim3((unsigned)blocks), dim3(THREADS), lds, st, (int)d, C, vec4, items, a, b, n_nodes, E,
                               lde, dlogits, dw_part);
        }
        const int64_t nout = (int64_t)C * d + C;
        hipLaunchKernelGGL(cls_dw_reduce_kernel, dim3((unsigned)((nout + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (int)d, C, blocks,
                           (const double *)dw_part, dW, db);
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
