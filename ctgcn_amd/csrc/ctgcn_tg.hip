// ctgcn_tg.hip — the PyTorch-Geometric variants of the GCN, GAT, GraphSAGE and GIN baselines (reference baseline/gcn.py, gat.py,
// sage.py, gin.py: TgGCN, TgGAT, TgSAGE, TgGIN) on the GPU: the operator of a raw [2, E] edge index, and the SAGE / GIN step.
// (TgGCN's step is ctgcn_gcn.hip's conv over the looped operator; TgGAT's attention is ctgcn_gat.hip's ctgcn_tgat_* entry points.)
//
//   keys        key[e] = target * n + source of edge e, n * n (past every valid key) and the flag for an index outside [0, n)
//   csr count   over the sorted keys, one thread per node v: raw_ptr[v] = the first key >= v n (a binary search, so no atomics),
//               loop_at[v] = the entries of row v with a source below v, nloops[v] = the loops (v, v) the input holds
//   csr emit    one thread per sorted entry and one per node.  The pairs as given: col[e] = source, mean[e] = 1 / (entries of the
//               row).  The looped pattern of GCNConv / GATConv: every non-loop entry at its sorted position, exactly one loop per
//               node at its own, value dis_s dis_t with dis_v = c_v^-1/2 over the looped row lengths c_v, formed in fp64 and
//               rounded to fp32 once.  A repeated pair stays a repeated entry.
//   tg conv     Y[i] = epi(sum_e val[e] S[col[e]] + self_scale T[i] + b); epi none, or ReLU and counter-based dropout
//               (ctgcn_rng.h).  SAGEConv after its product of width 2 d (val = 1 / row length), GINConv after its Linear (val = 1,
//               T = S, self_scale = 1 + eps: the Linear commutes with the sum).
//   conv prep   the backward's one N x d pass: G = dY where y + b > 0 (y the saved output, or the sum before the bias with b given)
//               and the dropout draw, made again from the key, kept it; the bias gradient as per-block column sums added in block
//               order.
//
// The gather is the pull form of ctgcn_gather.h, as in ctgcn_pool.hip.  No float atomics; every sum has a fixed order, so repeated
// launches are bit-identical.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr int EPI_NONE = 0, EPI_RELU = 1;

// ------------------------------------------------------------------------------------------------ the operator of an edge index
__global__ __launch_bounds__(256) void tg_keys_kernel(int64_t E, int64_t n, const int64_t *__restrict__ src, const int64_t *__restrict__ dst,
                                                      int64_t *__restrict__ keys, int32_t *flag)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t s = src[e], t = dst[e];
    const bool ok = s >= 0 && s < n && t >= 0 && t < n;
    keys[e] = ok ? t * n + s : n * n;
    if (!ok) atomicOr(flag, 1);                                   // the same bit from every thread: no order to depend on
}

// the first position in [0, E) whose key is >= want
__device__ __forceinline__ int64_t lower_bound(const int64_t *keys, int64_t E, int64_t want)
{
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void tg_count_kernel(int64_t E, int64_t n, const int64_t *__restrict__ keys, int32_t *__restrict__ raw_ptr,
                                                       int32_t *__restrict__ loop_at, int32_t *__restrict__ nloops)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > n) return;
    const int64_t first = lower_bound(keys, E, v * n);
    raw_ptr[v] = (int32_t)first;
    if (v == n) return;
    const int64_t lo = lower_bound(keys, E, v * n + v), hi = lower_bound(keys, E, v * n + v + 1);
    loop_at[v] = (int32_t)(lo - first);
    nloops[v] = (int32_t)(hi - lo);
}

__device__ __forceinline__ double dis_of(const int32_t *looped_ptr, int64_t v) { return 1.0 / sqrt((double)(looped_ptr[v + 1] - looped_ptr[v])); }

// threads [0, E): the sorted entries; threads [E, E + n): the nodes' loops
__global__ __launch_bounds__(256) void tg_emit_kernel(int64_t E, int64_t n, const int64_t *__restrict__ keys, const int32_t *__restrict__ raw_ptr,
                                                      const int32_t *__restrict__ loop_at, const int32_t *__restrict__ nloops,
                                                      const int32_t *__restrict__ looped_ptr, int32_t *__restrict__ col, float *__restrict__ mean,
                                                      int32_t *__restrict__ col_l, float *__restrict__ val_l)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E + n) return;
    if (idx >= E) {
        const int64_t v = idx - E;
        const int64_t at = (int64_t)looped_ptr[v] + loop_at[v];
        const double dis = dis_of(looped_ptr, v);
        col_l[at] = (int32_t)v;
        val_l[at] = (float)(dis * dis);
        return;
    }
    const int64_t k = keys[idx];
    if (k >= n * n) return;                                       // an index out of range: the flag is set and the caller raises
    const int64_t t = k / n, s = k - t * n;
    col[idx] = (int32_t)s;
    mean[idx] = (float)(1.0 / (double)(raw_ptr[t + 1] - raw_ptr[t]));
    if (s == t) return;
    int64_t pos = idx - raw_ptr[t];
    if (s > t) pos += 1 - nloops[t];                              // the input's loops leave, the row's one loop enters
    const int64_t at = (int64_t)looped_ptr[t] + pos;
    col_l[at] = (int32_t)s;
    val_l[at] = (float)(dis_of(looped_ptr, s) * dis_of(looped_ptr, t));
}

int check_graph(const char *what, int64_t E, int64_t n)
{
    if (E < 0 || n < 0 || n > INT32_MAX || E >= ((int64_t)1 << 31) - n) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and 0 <= E < 2^31 - n");
    return CTGCN_OK;
}

// ------------------------------------------------------------------------------------------------ tg conv
struct TgArgs {
    int64_t n;
    int32_t d, chunks;
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    const float *src;       // S
    int64_t ldsrc;
    const float *self;      // T or null
    int64_t ldself;
    float self_scale;
    const float *bias;      // [d] or null
    float *out;
    int64_t ldout;
    int32_t epi, drop;
    double p;
    float scale;            // 1 / (1 - p)
    uint64_t key;
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t max_pieces;
    int32_t part_ld;        // floats per partial vector: d rounded up to 4
    float *part;            // [n_long][max_pieces][part_ld]
};

// the entries lo, lo + step, ... below hi of a row
template <int VEC>
__device__ __forceinline__ typename vec_of<VEC>::type gather(const TgArgs &a, int lo, int hi, int step, int64_t foff)
{
    using V = typename vec_of<VEC>::type;
    V acc = V(0.f);
#pragma unroll 4
    for (int e = lo; e < hi; e += step) acc = vfma(a.val[e], *(const V *)(a.src + (int64_t)a.col[e] * a.ldsrc + foff), acc);
    return acc;
}

// the self term, the bias and the epilogue onto a finished sum
template <int VEC>
__device__ __forceinline__ void finish(const TgArgs &a, int64_t row, int64_t foff, typename vec_of<VEC>::type acc)
{
    using V = typename vec_of<VEC>::type;
    if (a.self) acc = vfma(a.self_scale, *(const V *)(a.self + row * a.ldself + foff), acc);
    float *y = (float *)&acc;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if (a.bias) y[k] += a.bias[foff + k];
        if (a.epi == EPI_RELU) {
            y[k] = y[k] > 0.f ? y[k] : 0.f;
            if (a.drop) y[k] = ctgcn_u01(a.key, (uint64_t)row, (uint64_t)(foff + k)) >= a.p ? y[k] * a.scale : 0.f;
        }
    }
    *(V *)(a.out + row * a.ldout + foff) = acc;
}

// every row that is not long
template <int VEC, int LPR>
__global__ __launch_bounds__(256) void tg_row_kernel(const TgArgs a)
{
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    const int start = a.row_ptr[row], end = a.row_ptr[row + 1];
    if (a.n_long > 0 && end - start > a.long_thresh) return;      // long row: tg_piece_kernel + tg_final_kernel
    for (int ch = lig; ch < a.chunks; ch += LPR) {
        const int64_t foff = (int64_t)ch * VEC;
        finish<VEC>(a, row, foff, gather<VEC>(a, start, end, 1, foff));
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of long row i into part[i][p]; its eight lane groups take interleaved entries
// and are added in group order
template <int VEC>
__global__ __launch_bounds__(PIECE_THREADS) void tg_piece_kernel(const TgArgs a)
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
        const int64_t foff = live ? (int64_t)ch * VEC : 0;        // dead lanes read chunk 0 (valid memory) and never store
        sm[g][lig] = gather<VEC>(a, lo + g, hi, PIECE_GROUPS, foff);
        __syncthreads();
        if (g == 0 && live) {
            V t = sm[0][lig];
#pragma unroll
            for (int q = 1; q < PIECE_GROUPS; ++q) t += sm[q][lig];
            *(V *)(dst + foff) = t;
        }
        __syncthreads();
    }
}

// one wave per long row: the pieces in piece order, then what the row kernel does with a finished sum
__global__ __launch_bounds__(64) void tg_final_kernel(const TgArgs a)
{
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        float t = src[c];
        for (int p = 1; p < np; ++p) t += src[(int64_t)p * a.part_ld + c];
        finish<1>(a, row, c, t);
    }
}

template <int VEC>
int launch(TgArgs a, hipStream_t st)
{
    a.chunks = a.d / VEC;                                         // VEC 4 only when d % 4 == 0
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((tg_row_kernel<VEC, decltype(lpr)::value>), grid, dim3(256), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(tg_piece_kernel<VEC>, grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(tg_final_kernel, grid, dim3(64), 0, st, a); });
}

// ------------------------------------------------------------------------------------------------ conv prep
// PREP_ROWS rows a block, one partial column-sum vector per block; colsum_kernel (ctgcn_gather.h) adds them in block order
struct PrepArgs {
    int64_t n;
    int32_t d, chunks, epi, drop;
    const float *dY;
    int64_t lddy;
    const float *Y;         // with an epilogue: the values whose sign (after the bias) the ReLU saw
    int64_t ldy;
    const float *bias;      // added to Y before the test; null when Y already holds it
    double p;
    float scale;
    uint64_t key;
    float *G;               // written with an epilogue; without one G is dY
    int64_t ldg;
    float *part;            // [blocks][part_ld] or null
    int32_t part_ld;
};

template <int VEC>
__global__ __launch_bounds__(64 * PREP_WAVES) void tg_prep_kernel(const PrepArgs a)
{
    using V = typename vec_of<VEC>::type;
    __shared__ V sm[PREP_WAVES][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    for (int p0 = 0; p0 < a.chunks; p0 += 64) {
        const int ch = p0 + lane;
        const bool live = ch < a.chunks;
        const int64_t foff = (int64_t)ch * VEC;
        V acc = V(0.f);
        if (live) {
            for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
                const int64_t r = row0 + k;
                V gv = *(const V *)(a.dY + r * a.lddy + foff);
                if (a.epi == EPI_RELU) {
                    const V yv = *(const V *)(a.Y + r * a.ldy + foff);
                    float *g = (float *)&gv;
                    const float *y = (const float *)&yv;
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        const float pre = a.bias ? y[q] + a.bias[foff + q] : y[q];
                        if (!(pre > 0.f)) g[q] = 0.f;
                        else if (a.drop) g[q] = ctgcn_u01(a.key, (uint64_t)r, (uint64_t)(foff + q)) >= a.p ? g[q] * a.scale : 0.f;
                    }
                    *(V *)(a.G + r * a.ldg + foff) = gv;
                }
                acc += gv;
            }
        }
        if (a.part) {                                             // block-uniform
            sm[w][lane] = acc;
            __syncthreads();
            if (w == 0 && live) {
                for (int k = 1; k < PREP_WAVES; ++k) acc += sm[k][lane];
                *(V *)(a.part + (int64_t)blockIdx.x * a.part_ld + foff) = acc;
            }
            __syncthreads();
        }
    }
}

int64_t prep_blocks(int64_t n) { return (n + PREP_ROWS - 1) / PREP_ROWS; }

}  // namespace

extern "C" int ctgcn_tg_keys(int64_t E, int64_t n, const int64_t *src, const int64_t *dst, int64_t *keys, int32_t *flag, void *stream)
{
    const char *what = "tg_keys";
    if (int rc = check_graph(what, E, n)) return rc;
    if (E == 0) return CTGCN_OK;
    if (!src || !dst || !keys || !flag) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipLaunchKernelGGL(tg_keys_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, E, n, src, dst, keys, flag);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_tg_csr_count(int64_t E, int64_t n, const int64_t *keys, int32_t *raw_ptr, int32_t *loop_at, int32_t *nloops, void *stream)
{
    const char *what = "tg_csr_count";
    if (int rc = check_graph(what, E, n)) return rc;
    if (!raw_ptr || (E > 0 && !keys) || (n > 0 && (!loop_at || !nloops))) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipLaunchKernelGGL(tg_count_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, E, n, keys, raw_ptr, loop_at, nloops);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_tg_csr_emit(int64_t E, int64_t n, const int64_t *keys, const int32_t *raw_ptr, const int32_t *loop_at, const int32_t *nloops,
                                 const int32_t *looped_ptr, int32_t *col, float *mean, int32_t *col_l, float *val_l, void *stream)
{
    const char *what = "tg_csr_emit";
    if (int rc = check_graph(what, E, n)) return rc;
    if (E + n == 0) return CTGCN_OK;
    if (!raw_ptr || !looped_ptr || (n > 0 && (!loop_at || !nloops || !col_l || !val_l)) || (E > 0 && (!keys || !col || !mean)))
        return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipLaunchKernelGGL(tg_emit_kernel, dim3((unsigned)((E + n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, E, n, keys, raw_ptr, loop_at, nloops,
                       looped_ptr, col, mean, col_l, val_l);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_tg_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                     int64_t lds, const float *T, int64_t ldt, float self_scale, const float *bias, float *Y, int64_t ldy,
                                     int32_t epi, double p, uint64_t key, const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "tg_conv_fwd";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (epi != EPI_NONE && epi != EPI_RELU) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none) or 1 (ReLU, dropout)");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (lds < d || ldy < d || (T && ldt < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val || !S || !Y) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    TgArgs a{};
    a.n = n; a.d = d; a.row_ptr = row_ptr; a.col = col; a.val = val; a.src = S; a.ldsrc = lds; a.self = T; a.ldself = ldt;
    a.self_scale = self_scale; a.bias = bias; a.out = Y; a.ldout = ldy; a.epi = epi; a.drop = epi == EPI_RELU && p > 0.0; a.p = p;
    a.scale = 1.0f / (1.0f - (float)p); a.key = key; a.part_ld = (d + 3) & ~3;
    if (int rc = set_long_rows(a, what, long_rows, n_long, long_threshold, (size_t)a.part_ld, workspace, workspace_bytes,
                               "long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes, one piece per row"))
        return rc;
    return float4_rows(d, {{S, lds}, {T, ldt}, {Y, ldy}}) ? launch<4>(a, (hipStream_t)stream) : launch<1>(a, (hipStream_t)stream);
}

extern "C" size_t ctgcn_tg_prep_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 0 || d < 1) return 0;
    return (size_t)prep_blocks(n) * (size_t)((d + 3) & ~3) * sizeof(float);
}

extern "C" int ctgcn_tg_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *bias,
                                      int32_t epi, double p, uint64_t key, float *G, int64_t ldg, float *db, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    const char *what = "tg_conv_prep";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (epi != EPI_NONE && epi != EPI_RELU) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none) or 1 (ReLU, dropout)");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (lddy < d || (epi == EPI_RELU && (ldy < d || ldg < d))) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n == 0) return CTGCN_OK;
    if (!dY || (epi == EPI_RELU && (!Y || !G))) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (epi == EPI_NONE && !db) return ctgcn_fail(CTGCN_E_INVALID, what, "nothing to compute: no epilogue and no bias gradient");
    if (db && (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < ctgcn_tg_prep_workspace_bytes(n, d)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "a bias gradient needs a 16-byte aligned workspace of ctgcn_tg_prep_workspace_bytes() bytes");
    PrepArgs a{};
    a.n = n; a.d = d; a.epi = epi; a.drop = epi == EPI_RELU && p > 0.0; a.dY = dY; a.lddy = lddy; a.Y = Y; a.ldy = ldy; a.bias = bias; a.p = p;
    a.scale = 1.0f / (1.0f - (float)p); a.key = key; a.G = G; a.ldg = ldg; a.part = db ? (float *)workspace : nullptr; a.part_ld = (d + 3) & ~3;
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = prep_blocks(n);
    const bool v4 = epi == EPI_RELU ? float4_rows(d, {{dY, lddy}, {Y, ldy}, {G, ldg}}) : float4_rows(d, {{dY, lddy}});
    a.chunks = v4 ? d / 4 : d;
    if (v4) hipLaunchKernelGGL(tg_prep_kernel<4>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    else hipLaunchKernelGGL(tg_prep_kernel<1>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    if (db) {
        hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), dim3((unsigned)((d + DB_COLS - 1) / DB_COLS)), dim3(DB_COLS * DB_SEGS), 0, st, blocks, d,
                           a.part_ld, (const float *)a.part, db);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}
