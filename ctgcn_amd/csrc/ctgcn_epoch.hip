// ctgcn_epoch.hip — one epoch of the reference's unsupervised schedule (embedding.py:330-368) in a few launches per snapshot.
//
// Inside an epoch the weights do not change and the forward is deterministic, so every batch sees the same embeddings E and
// Σ_b ∇L_b(W) is the gradient of Σ_b L_b from ONE forward/backward.  This file supplies the per-snapshot pieces:
//   - the negative-sampling draws of all batches at once (bit-identical to ctgcn_neg_sampling_indices per batch);
//   - the negative-sampling loss (metrics.py:38-66) of all batches, forward and dE in one pass over the samples, no [S, d] gathers;
//   - the reconstruction loss of the -S models (metrics.py:111-123) under the epoch partition.
// Every gradient row is written by exactly one wave per kernel (no float atomics): dE is bit-identical from call to call.
// Positions p = 0..P-1 index the epoch permutation; batch b holds positions [b·bs, min((b+1)·bs, P)).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "ctgcn_logreg.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAXC = 8;             // columns per lane: d <= 512
constexpr int SCAN_T = 256, SCAN_PER = 8, SCAN_TILE = SCAN_T * SCAN_PER;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

// exclusive scan of 256 values held one per thread (Hillis-Steele in LDS); returns the thread's exclusive prefix, *total the sum
__device__ int64_t block_exclusive_scan(int64_t v, int64_t *sh, int64_t *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const int64_t add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[SCAN_T - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ int64_t take_of(int64_t p, int64_t P, const int64_t *perm, const int32_t *row_ptr, int num)
{
    if (p >= P) return 0;
    const int64_t v = perm[p];
    return min((int64_t)(row_ptr[v + 1] - row_ptr[v]), (int64_t)num);
}

// sample counts min(deg, num) of the positions: per-tile sums
__global__ __launch_bounds__(SCAN_T) void take_tile_sum_kernel(int64_t P, const int64_t *__restrict__ perm, const int32_t *__restrict__ row_ptr,
                                                               int num, int64_t *__restrict__ tile_sum)
{
    __shared__ int64_t sh[SCAN_T];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    int64_t s = 0;
    for (int i = 0; i < SCAN_PER; ++i) s += take_of(base + i, P, perm, row_ptr, num);
    int64_t total;
    block_exclusive_scan(s, sh, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: exclusive scan of the tile sums in place; tile_sum[ntiles] = grand total, also written to offsets[P]
__global__ __launch_bounds__(SCAN_T) void tile_scan_kernel(int64_t ntiles, int64_t *__restrict__ tile_sum, int64_t *__restrict__ total_out)
{
    __shared__ int64_t sh[SCAN_T];
    int64_t carry = 0;
    for (int64_t c = 0; c < ntiles; c += SCAN_T) {
        const int64_t i = c + threadIdx.x;
        const int64_t v = i < ntiles ? tile_sum[i] : 0;
        int64_t total;
        const int64_t ex = block_exclusive_scan(v, sh, &total);
        if (i < ntiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { tile_sum[ntiles] = carry; *total_out = carry; }
}

__global__ __launch_bounds__(SCAN_T) void take_offsets_kernel(int64_t P, const int64_t *__restrict__ perm, const int32_t *__restrict__ row_ptr,
                                                              int num, const int64_t *__restrict__ tile_prefix, int64_t *__restrict__ offsets)
{
    __shared__ int64_t sh[SCAN_T];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    int64_t v[SCAN_PER], s = 0;
    for (int i = 0; i < SCAN_PER; ++i) { v[i] = take_of(base + i, P, perm, row_ptr, num); s += v[i]; }
    int64_t total;
    int64_t o = tile_prefix[blockIdx.x] + block_exclusive_scan(s, sh, &total);
    for (int i = 0; i < SCAN_PER && base + i < P; ++i) { offsets[base + i] = o; o += v[i]; }
}

__global__ __launch_bounds__(256) void batch_offsets_kernel(int64_t P, int64_t bs, int64_t nb, const int64_t *__restrict__ offsets,
                                                            int64_t *__restrict__ batch_off)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > nb) return;
    batch_off[b] = offsets[min(b * bs, P)];
}

// pos_sample_kernel (ctgcn_walks.hip) for every batch at once: the draw of position p is keyed on (seeds[p / bs], p mod bs, k)
__global__ __launch_bounds__(256) void pos_sample_batched_kernel(int64_t P, const int64_t *__restrict__ perm, int64_t bs,
                                                                 const uint64_t *__restrict__ seeds, const int32_t *__restrict__ row_ptr,
                                                                 const int32_t *__restrict__ col, int num, const int64_t *__restrict__ offsets,
                                                                 int64_t *__restrict__ node_out, int64_t *__restrict__ pos_out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int64_t b = p / bs, local = p - b * bs;
    const uint64_t seed = seeds[b];
    const int64_t v = perm[p];
    const int s = row_ptr[v], deg = row_ptr[v + 1] - s;
    int64_t o = offsets[p];
    int need = min(deg, num);
    for (int k = 0; k < deg && need > 0; ++k) {
        const bool take = (deg <= num) || (ctgcn_u01(seed, (uint64_t)local, (uint64_t)k) * (double)(deg - k) < (double)need);
        if (take) { node_out[o] = v; pos_out[o] = col[s + k]; ++o; --need; }
    }
}

// neg_sample_kernel (ctgcn_walks.hip) for every batch at once: one thread per batch, row b of neg_out / scratch
__global__ __launch_bounds__(64) void neg_sample_batched_kernel(int64_t nb, int64_t table_len, const int32_t *__restrict__ table, int num,
                                                                const uint64_t *__restrict__ seeds, int64_t *__restrict__ neg_out,
                                                                int64_t *__restrict__ scratch)
{
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const uint64_t seed = seeds[b] ^ 0xabcdefull;
    int64_t *pos = scratch + b * num;
    int64_t *out = neg_out + b * num;
    int got = 0;
    for (uint64_t tries = 0; got < num; ++tries) {
        const int64_t p = min((int64_t)(ctgcn_u01(seed, 0x5eedull, tries) * (double)table_len), table_len - 1);
        bool dup = false;
        for (int i = 0; i < got; ++i) dup |= (pos[i] == p);
        if (!dup) { pos[got] = p; out[got] = table[p]; ++got; }
    }
}

__device__ __forceinline__ int64_t batch_end(int64_t b, int64_t bs, int64_t P) { return min((b + 1) * bs, P); }

// S_b = Σ_j E[neg[b, j]] in j order (block per batch)
__global__ __launch_bounds__(256) void neg_sum_kernel(int d, int num, const float *__restrict__ E, int64_t lde, const int64_t *__restrict__ neg,
                                                      float *__restrict__ S)
{
    const int64_t b = blockIdx.x;
    for (int c = threadIdx.x; c < d; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < num; ++j) acc += E[neg[b * num + j] * lde + c];
        S[b * d + c] = acc;
    }
}

// one wave per position p (node u, samples s0..s1): pos_s = e_u·e_v, neg = e_u·S_b (the same for all of u's samples);
// dE[u] += Σ_s gpos_s e_v + Σ_s gneg S_b.  Saves gpos_s (the positives' scatter), G_p = Σ_s gneg (dS_b) and the loss partial.
__global__ __launch_bounds__(256) void negloss_node_kernel(int64_t P, int64_t bs, int d, float Q, const float *__restrict__ E, int64_t lde,
                                                           const int64_t *__restrict__ offsets, const int64_t *__restrict__ node_idx,
                                                           const int64_t *__restrict__ pos_idx, const float *__restrict__ S,
                                                           float *__restrict__ gpos, float *__restrict__ G, double *__restrict__ lossp,
                                                           float *__restrict__ dE, int64_t ldg)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t p = (int64_t)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
    if (p >= P) return;
    const int64_t s0 = offsets[p], s1 = offsets[p + 1];
    if (s0 == s1) {
        if (lane == 0) { G[p] = 0.f; lossp[p] = 0.0; }
        return;
    }
    const int64_t b = p / bs;
    const double inv_n = 1.0 / (double)(offsets[batch_end(b, bs, P)] - offsets[b * bs]);
    const int64_t u = node_idx[s0];
    float eu[MAXC], sb[MAXC], acc[MAXC];
    float dn = 0.f;
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
        const int c = lane + k * WAVE;
        eu[k] = c < d ? E[u * lde + c] : 0.f;
        sb[k] = c < d ? S[b * d + c] : 0.f;
        acc[k] = 0.f;
        dn += eu[k] * sb[k];
    }
    dn = wave_sum(dn);
    double lpos = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t v = pos_idx[s];
        float ev[MAXC], dp = 0.f;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            const int c = lane + k * WAVE;
            ev[k] = c < d ? E[v * lde + c] : 0.f;
            dp += eu[k] * ev[k];
        }
        dp = wave_sum(dp);
        lpos += softplus(-(double)dp);
        const float gp = (float)(-sigmoid(-(double)dp) * inv_n);       // d/dx mean softplus(-x)
#pragma unroll
        for (int k = 0; k < MAXC; ++k) acc[k] += gp * ev[k];
        if (lane == 0) gpos[s] = gp;
    }
    const double cnt = (double)(s1 - s0);
    const float gn = (float)((double)Q * sigmoid((double)dn) * inv_n * cnt);   // Σ over u's samples of d/dx Q·mean softplus(x)
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
        const int c = lane + k * WAVE;
        if (c < d) dE[u * ldg + c] += acc[k] + gn * sb[k];
    }
    if (lane == 0) {
        G[p] = gn;
        lossp[p] = (lpos + (double)Q * cnt * softplus((double)dn)) * inv_n;
    }
}

// block per batch: loss_b = Σ_p lossp[p] (fixed tree), and with G != NULL dS_b = Σ_p G_p e_{u_p} (4 waves, combined in wave order)
__global__ __launch_bounds__(256) void batch_reduce_kernel(int64_t P, int64_t bs, int d, const double *__restrict__ lossp, double *__restrict__ loss_out,
                                                           const float *__restrict__ G, const int64_t *__restrict__ offsets,
                                                           const int64_t *__restrict__ node_idx, const float *__restrict__ E, int64_t lde,
                                                           float *__restrict__ dS)
{
    __shared__ double shl[256];
    __shared__ float shs[4][MAXC * WAVE];
    const int64_t b = blockIdx.x, p0 = b * bs, p1 = batch_end(b, bs, P);
    double l = 0.0;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) l += lossp[p];
    shl[threadIdx.x] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) shl[threadIdx.x] += shl[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[b] = shl[0];
    if (!G) return;
    const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
    float acc[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; ++k) acc[k] = 0.f;
    for (int64_t p = p0 + w; p < p1; p += 4) {
        if (offsets[p] == offsets[p + 1]) continue;
        const float g = G[p];
        const int64_t u = node_idx[offsets[p]];
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            const int c = lane + k * WAVE;
            if (c < d) acc[k] += g * E[u * lde + c];
        }
    }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) shs[w][lane + k * WAVE] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) dS[b * d + c] = ((shs[0][c] + shs[1][c]) + shs[2][c]) + shs[3][c];
}

// segmented reduction over a stably sorted index: for every run of equal keys, G[key] += Σ_j coef[src_j] · M[row(src_j)]
// in sorted order, src_j = order[j], row = rowmap ? rowmap[src] : src / row_div, coef = 1 without coefs.  One wave per run head.
__global__ __launch_bounds__(256) void segment_rows_kernel(int64_t m, int d, const int64_t *__restrict__ keys, const int64_t *__restrict__ order,
                                                           const float *__restrict__ coefs, const int64_t *__restrict__ rowmap, int64_t row_div,
                                                           const float *__restrict__ M, int64_t ldm, float *__restrict__ G, int64_t ldg)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t i = (int64_t)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
    if (i >= m) return;
    const int64_t key = keys[i];
    if (i > 0 && keys[i - 1] == key) return;
    float acc[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; ++k) acc[k] = 0.f;
    for (int64_t j = i; j < m && keys[j] == key; ++j) {
        const int64_t src = order[j];
        const int64_t row = rowmap ? rowmap[src] : src / row_div;
        const float cf = coefs ? coefs[src] : 1.f;
#pragma unroll
        for (int k = 0; k < MAXC; ++k) {
            const int c = lane + k * WAVE;
            if (c < d) acc[k] += cf * M[row * ldm + c];
        }
    }
#pragma unroll
    for (int k = 0; k < MAXC; ++k) {
        const int c = lane + k * WAVE;
        if (c < d) G[key * ldg + c] += acc[k];
    }
}

// one wave per position: row r = rows[p] of batch b, w = 1 / (|b| d): loss partial w Σ (s - e)², ds = 2 w (s - e), de = -ds
__global__ __launch_bounds__(256) void recon_row_kernel(int64_t P, int64_t bs, int d, const int64_t *__restrict__ rows, const float *__restrict__ S,
                                                        int64_t lds, const float *__restrict__ E, int64_t lde, double *__restrict__ lossp,
                                                        float *__restrict__ dS, int64_t ldds, float *__restrict__ dE, int64_t ldde)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t p = (int64_t)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
    if (p >= P) return;
    const int64_t b = p / bs;
    const double w = 1.0 / ((double)(batch_end(b, bs, P) - b * bs) * (double)d);
    const int64_t r = rows[p];
    double part = 0.0;
    for (int c = lane; c < d; c += WAVE) {
        const float diff = S[r * lds + c] - E[r * lde + c];
        part += (double)diff * (double)diff;
        const float g = (float)(2.0 * w * (double)diff);
        if (dS) dS[r * ldds + c] += g;
        if (dE) dE[r * ldde + c] -= g;
    }
    part = wave_sum(part);
    if (lane == 0) lossp[p] = part * w;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct NegLossWs {
    float *S, *dS, *gpos, *G;
    double *lossp;
};
size_t negloss_ws(int64_t P, int64_t samples, int64_t nb, int32_t d, char *base, NegLossWs *w)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + o : nullptr; o += align256(bytes); return q; };
    char *S = take((size_t)nb * d * sizeof(float)), *dS = take((size_t)nb * d * sizeof(float));
    char *gpos = take((size_t)samples * sizeof(float)), *G = take((size_t)P * sizeof(float)), *lossp = take((size_t)P * sizeof(double));
    if (w) *w = NegLossWs{(float *)S, (float *)dS, (float *)gpos, (float *)G, (double *)lossp};
    return o;
}

}  // namespace

extern "C" size_t ctgcn_epoch_scan_workspace_bytes(int64_t positions)
{
    return positions < 0 ? 0 : (size_t)(ceil_div(positions, SCAN_TILE) + 1) * sizeof(int64_t);
}

extern "C" int ctgcn_neg_sampling_offsets_batched(int64_t positions, const int64_t *perm, const int32_t *pair_row_ptr, int32_t num,
                                                  int64_t batch_size, int64_t *offsets, int64_t *batch_offsets, void *workspace,
                                                  size_t workspace_bytes, void *stream)
{
    if (positions < 0 || num < 1 || batch_size < 1) return ctgcn_set_error_(CTGCN_E_INVALID, "neg_sampling_offsets_batched: bad sizes");
    if (!offsets || !batch_offsets || (positions > 0 && (!perm || !pair_row_ptr || !workspace)))
        return ctgcn_set_error_(CTGCN_E_INVALID, "neg_sampling_offsets_batched: null pointer");
    if (workspace_bytes < ctgcn_epoch_scan_workspace_bytes(positions))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "neg_sampling_offsets_batched: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = ceil_div(positions, batch_size);
    if (positions == 0) {
        CTGCN_TRY(hipMemsetAsync(offsets, 0, sizeof(int64_t), st));
        CTGCN_TRY(hipMemsetAsync(batch_offsets, 0, sizeof(int64_t), st));
        return CTGCN_OK;
    }
    const int64_t ntiles = ceil_div(positions, SCAN_TILE);
    if (ntiles > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "neg_sampling_offsets_batched: too many positions");
    int64_t *tiles = (int64_t *)workspace;
    hipLaunchKernelGGL(take_tile_sum_kernel, dim3((unsigned)ntiles), dim3(SCAN_T), 0, st, positions, perm, pair_row_ptr, (int)num, tiles);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(SCAN_T), 0, st, ntiles, tiles, offsets + positions);
    hipLaunchKernelGGL(take_offsets_kernel, dim3((unsigned)ntiles), dim3(SCAN_T), 0, st, positions, perm, pair_row_ptr, (int)num, tiles, offsets);
    hipLaunchKernelGGL(batch_offsets_kernel, dim3((unsigned)ceil_div(nb + 1, 256)), dim3(256), 0, st, positions, batch_size, nb, offsets, batch_offsets);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_neg_sampling_indices_batched(int64_t positions, const int64_t *perm, int64_t batch_size, const uint64_t *seeds,
                                                  const int32_t *pair_row_ptr, const int32_t *pair_col, int32_t num, int64_t table_len,
                                                  const int32_t *neg_table, const int64_t *offsets, int64_t *node_out, int64_t *pos_out,
                                                  int64_t *neg_out, int64_t *scratch, void *stream)
{
    if (positions < 0 || batch_size < 1 || num < 1 || table_len < num)
        return ctgcn_set_error_(CTGCN_E_INVALID, "neg_sampling_indices_batched: bad sizes (the negative table must hold at least `num` entries)");
    if (positions == 0) return CTGCN_OK;
    if (!perm || !seeds || !pair_row_ptr || !neg_table || !offsets || !neg_out || !scratch)
        return ctgcn_set_error_(CTGCN_E_INVALID, "neg_sampling_indices_batched: null pointer");
    const int64_t nb = ceil_div(positions, batch_size);
    hipStream_t st = (hipStream_t)stream;
    if (node_out && pos_out)         // NULL when the window has no samples at all (the caller skips the allocation)
        hipLaunchKernelGGL(pos_sample_batched_kernel, dim3((unsigned)ceil_div(positions, 256)), dim3(256), 0, st, positions, perm, batch_size,
                           seeds, pair_row_ptr, pair_col, (int)num, offsets, node_out, pos_out);
    hipLaunchKernelGGL(neg_sample_batched_kernel, dim3((unsigned)ceil_div(nb, 64)), dim3(64), 0, st, nb, table_len, neg_table, (int)num, seeds,
                       neg_out, scratch);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_negsampling_loss_workspace_bytes(int64_t positions, int64_t samples, int64_t batch_size, int32_t d)
{
    if (positions < 0 || samples < 0 || batch_size < 1 || d < 1) return 0;
    return negloss_ws(positions, samples, ceil_div(positions, batch_size), d, nullptr, nullptr);
}

extern "C" int ctgcn_negsampling_loss_fwd_bwd_f32(int64_t positions, int64_t batch_size, int64_t samples, int32_t d, int32_t num, float Q,
                                                  const float *E, int64_t lde, const int64_t *offsets, const int64_t *node_idx,
                                                  const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *pos_sorted,
                                                  const int64_t *pos_order, const int64_t *neg_sorted, const int64_t *neg_order,
                                                  double *loss_out, float *dE, int64_t ldg, void *workspace, size_t workspace_bytes,
                                                  void *stream)
{
    if (positions < 0 || batch_size < 1 || samples < 0 || d < 1 || num < 1 || lde < d || ldg < d)
        return ctgcn_set_error_(CTGCN_E_INVALID, "negsampling_loss_fwd_bwd: bad sizes");
    if (d > MAXC * WAVE) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "negsampling_loss_fwd_bwd: d > 512");
    if (positions == 0) return CTGCN_OK;
    if (!E || !offsets || !neg_idx || !neg_sorted || !neg_order || !loss_out || !dE || !workspace ||
        (samples > 0 && (!node_idx || !pos_idx || !pos_sorted || !pos_order)))
        return ctgcn_set_error_(CTGCN_E_INVALID, "negsampling_loss_fwd_bwd: null pointer");
    if (workspace_bytes < ctgcn_negsampling_loss_workspace_bytes(positions, samples, batch_size, d))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "negsampling_loss_fwd_bwd: workspace too small");
    const int64_t nb = ceil_div(positions, batch_size);
    if (ceil_div(positions, 4) > 0x7fffffffLL || ceil_div(samples, 4) > 0x7fffffffLL || nb > 0x7fffffffLL)
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "negsampling_loss_fwd_bwd: too many positions / samples");
    hipStream_t st = (hipStream_t)stream;
    NegLossWs w;
    negloss_ws(positions, samples, nb, d, (char *)workspace, &w);
    hipLaunchKernelGGL(neg_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, (int)d, (int)num, E, lde, neg_idx, w.S);
    hipLaunchKernelGGL(negloss_node_kernel, dim3((unsigned)ceil_div(positions, 4)), dim3(256), 0, st, positions, batch_size, (int)d, Q, E, lde,
                       offsets, node_idx, pos_idx, w.S, w.gpos, w.G, w.lossp, dE, ldg);
    hipLaunchKernelGGL(batch_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, positions, batch_size, (int)d, w.lossp, loss_out, w.G, offsets,
                       node_idx, E, lde, w.dS);
    if (samples > 0)        // dE[v] += Σ gpos_s e_{u_s} over the samples whose positive is v
        hipLaunchKernelGGL(segment_rows_kernel, dim3((unsigned)ceil_div(samples, 4)), dim3(256), 0, st, samples, (int)d, pos_sorted, pos_order,
                           (const float *)w.gpos, node_idx, (int64_t)1, (const float *)E, lde, dE, ldg);
    // dE[neg_{b,j}] += dS_b over every (b, j) (collisions across batches and within one: one run per node)
    hipLaunchKernelGGL(segment_rows_kernel, dim3((unsigned)ceil_div(nb * num, 4)), dim3(256), 0, st, nb * num, (int)d, neg_sorted, neg_order,
                       (const float *)nullptr, (const int64_t *)nullptr, (int64_t)num, (const float *)w.dS, (int64_t)d, dE, ldg);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_reconstruction_loss_workspace_bytes(int64_t positions)
{
    return positions < 0 ? 0 : align256((size_t)positions * sizeof(double));
}

extern "C" int ctgcn_reconstruction_loss_fwd_bwd_f32(int64_t positions, int64_t batch_size, int32_t d, const int64_t *rows, const float *S,
                                                     int64_t lds, const float *E, int64_t lde, double *loss_out, float *dS, int64_t ldds,
                                                     float *dE, int64_t ldde, void *workspace, size_t workspace_bytes, void *stream)
{
    if (positions < 0 || batch_size < 1 || d < 1 || lds < d || lde < d || (dS && ldds < d) || (dE && ldde < d))
        return ctgcn_set_error_(CTGCN_E_INVALID, "reconstruction_loss_fwd_bwd: bad sizes");
    if (positions == 0) return CTGCN_OK;
    if (!rows || !S || !E || !loss_out || !workspace) return ctgcn_set_error_(CTGCN_E_INVALID, "reconstruction_loss_fwd_bwd: null pointer");
    if (workspace_bytes < ctgcn_reconstruction_loss_workspace_bytes(positions))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "reconstruction_loss_fwd_bwd: workspace too small");
    if (ceil_div(positions, 4) > 0x7fffffffLL) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "reconstruction_loss_fwd_bwd: too many positions");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = ceil_div(positions, batch_size);
    double *lossp = (double *)workspace;
    hipLaunchKernelGGL(recon_row_kernel, dim3((unsigned)ceil_div(positions, 4)), dim3(256), 0, st, positions, batch_size, (int)d, rows, S, lds, E,
                       lde, lossp, dS, ldds, dE, ldde);
    hipLaunchKernelGGL(batch_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, positions, batch_size, (int)d, (const double *)lossp, loss_out,
                       (const float *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr, (const float *)nullptr, (int64_t)0,
                       (float *)nullptr);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
