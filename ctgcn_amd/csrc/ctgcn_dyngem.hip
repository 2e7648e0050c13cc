// ctgcn_dyngem.hip — the passes of the DynGEM and DynAE baselines (reference baseline/dynGEM.py, baseline/dynAE.py) over a window of
// snapshots held as one stacked CSR (ops.SnapshotRows: row t N + v is row v of snapshot t, columns are node ids).  The reference feeds
// dense adjacency rows to an MLP; nothing here forms one.
//
//   rowsel conv   Y[b] = epi(bias + sum_{s < L} sum_{e in row idx[b][s]} val[e] S[s col_stride + col[e]]): the first Linear of the encoder
//                 over the selected rows, as a gather.  On the scaffold of ctgcn_gather.h with batch positions in the role of rows: a
//                 position's entries are those of its L rows one after the other, a position of more than long_threshold entries is
//                 cut into pieces of that run.  No atomics, every sum has a fixed order.
//   bucket        out[r] = sum of G[b] over the batch positions b that selected stacked row r, in ascending b, from an inverted index.
//                 The backward of the gather is then the plain aggregation (ctgcn_gcn_conv_fwd_f32) of the buckets over the transposed
//                 stack.
//   wrecon loss   sum_b scale / div_b (sum_j p_bj² + sum_{stored j} (β² (p_bj − v_bj)² − p_bj²)), the reference's
//                 sum(((pred − x) penalty)²) with penalty β at x != 0 and 1 elsewhere, and its gradient, from one sweep of a row of the
//                 prediction and a correction at the target row's stored entries, both by the row's workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_try.h"

namespace {

constexpr int U = 4;                   // gathered rows in flight per lane group
constexpr int MAX_SLOTS = 64;          // rows a batch position may select (look_back)

__device__ __forceinline__ f4 relu_of(f4 v) { return f4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }
__device__ __forceinline__ float relu_of(float v) { return fmaxf(v, 0.f); }

struct RowselArgs {
    int64_t n;              // batch positions
    int32_t d, slots;
    const int32_t *idx;     // [n][slots] stacked row ids, -1 an empty row
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    const float *src;       // S; slot s gathers from the rows s col_stride + col
    int64_t ldsrc, col_stride;
    const float *bias;
    int32_t relu;
    float *out;
    int64_t ldout;
    const int32_t *long_rows;   // the long positions
    int32_t n_long, long_thresh;
    int32_t chunks, max_pieces, part_ld;
    float *part;            // [n_long][max_pieces][part_ld]
};

// entries of a position: those of its rows, slot after slot
__device__ __forceinline__ int64_t position_len(const RowselArgs &a, const int32_t *ix)
{
    int64_t len = 0;
    for (int s = 0; s < a.slots; ++s) {
        const int r = ix[s];
        if (r >= 0) len += a.row_ptr[r + 1] - a.row_ptr[r];
    }
    return len;
}

// P + sum_e val[e] src[col[e]][foff ..] over the entries [start, end) of a row, by the position's LPR lanes (ctgcn_gcn.hip's row_sum)
template <int VEC, int LPR>
__device__ __forceinline__ typename vec_of<VEC>::type row_sum(const RowselArgs &a, const float *src, int start, int end, int lig, int64_t foff,
                                                               typename vec_of<VEC>::type P)
{
    using V = typename vec_of<VEC>::type;
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
                xv[u] = *(const V *)(src + (int64_t)cj * a.ldsrc + foff);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) P = vfma(wj[u], xv[u], P);
        }
        for (; j < cnt; ++j) {
            const int cj = __shfl(c, j, LPR);
            const float w1 = __shfl(w, j, LPR);
            P = vfma(w1, *(const V *)(src + (int64_t)cj * a.ldsrc + foff), P);
        }
    }
    return P;
}

// every position that is not long
template <int VEC, int LPR>
__global__ __launch_bounds__(256) void rowsel_row_kernel(const RowselArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t pos = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (pos >= a.n) return;
    const int32_t *ix = a.idx + pos * a.slots;
    if (a.n_long > 0 && position_len(a, ix) > a.long_thresh) return;     // long position: rowsel_piece_kernel + rowsel_final_kernel
    for (int p0 = 0; p0 < a.chunks; p0 += LPR) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        // dead lanes read chunk 0 (valid memory) and never store: keeps every load unconditional
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
        for (int s = 0; s < a.slots; ++s) {
            const int r = ix[s];
            if (r < 0) continue;                                          // uniform over the position's lanes
            P = row_sum<VEC, LPR>(a, a.src + (int64_t)s * a.col_stride * a.ldsrc, a.row_ptr[r], a.row_ptr[r + 1], lig, foff, P);
        }
        if (a.bias) P += *(const V *)(a.bias + foff);
        if (a.relu) P = relu_of(P);
        if (live) *(V *)(a.out + pos * a.ldout + foff) = P;
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of the entry run of long position i into part[i][p]
template <int VEC>
__global__ __launch_bounds__(PIECE_THREADS) void rowsel_piece_kernel(const RowselArgs a)
{
    using V = typename vec_of<VEC>::type;
    __shared__ V sm[PIECE_GROUPS][PIECE_LANES];
    const int64_t pos = a.long_rows[blockIdx.y];
    const int32_t *ix = a.idx + pos * a.slots;
    const int64_t len = position_len(a, ix);
    const int np = pieces_of((int)(len > INT32_MAX ? INT32_MAX : len), a.long_thresh, a.max_pieces);
    const int p = blockIdx.x;
    if (p >= np) return;
    const int64_t plen = (len + np - 1) / np;
    const int64_t lo = min(len, p * plen), hi = min(len, (p + 1) * plen);
    const int lig = threadIdx.x & (PIECE_LANES - 1), g = threadIdx.x / PIECE_LANES;
    float *dst = a.part + ((int64_t)blockIdx.y * a.max_pieces + p) * a.part_ld;

    for (int p0 = 0; p0 < a.chunks; p0 += PIECE_LANES) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
        int64_t off = 0;                                                  // where slot s starts in the run
        for (int s = 0; s < a.slots; ++s) {
            const int r = ix[s];
            if (r < 0) continue;
            const int start = a.row_ptr[r];
            const int64_t slen = a.row_ptr[r + 1] - start;
            const int64_t k0 = max(lo, off), k1 = min(hi, off + slen);
            if (k0 < k1) {
                const float *src = a.src + (int64_t)s * a.col_stride * a.ldsrc;
                // group g takes the run's entries lo + g, lo + g + 8, ...
                int64_t k = k0 + ((g - (k0 - lo)) % PIECE_GROUPS + PIECE_GROUPS) % PIECE_GROUPS;
                for (; k < k1; k += PIECE_GROUPS) {
                    const int64_t e = start + (k - off);
                    P = vfma(a.val[e], *(const V *)(src + (int64_t)a.col[e] * a.ldsrc + foff), P);
                }
            }
            off += slen;
        }
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

// one wave per long position: the pieces in piece order, the bias, the epilogue
__global__ __launch_bounds__(64) void rowsel_final_kernel(const RowselArgs a)
{
    const int64_t pos = a.long_rows[blockIdx.x];
    const int64_t len = position_len(a, a.idx + pos * a.slots);
    const int np = pieces_of((int)(len > INT32_MAX ? INT32_MAX : len), a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        float t = src[c];
        for (int p = 1; p < np; ++p) t += src[(int64_t)p * a.part_ld + c];
        if (a.bias) t += a.bias[c];
        if (a.relu) t = fmaxf(t, 0.f);
        a.out[pos * a.ldout + c] = t;
    }
}

template <int VEC>
int launch_rowsel(RowselArgs a, hipStream_t st)
{
    a.chunks = (a.d + VEC - 1) / VEC;
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((rowsel_row_kernel<VEC, decltype(lpr)::value>), grid, dim3(256), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL((rowsel_piece_kernel<VEC>), grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(rowsel_final_kernel, grid, dim3(64), 0, st, a); });
}

// ------------------------------------------------------------------------------------------------ bucket sums of the backward
struct BucketArgs {
    int64_t rows;
    int32_t d, chunks;
    const int32_t *inv_ptr;  // [rows + 1]
    const int32_t *inv_pos;  // batch positions, ascending within a row
    const float *G;
    int64_t ldg;
    float *out;
    int64_t ldout;
};

// LPR lanes own a stacked row and a float4 (or a float) per lane of it; a row nobody selected is written as zeros
template <int VEC, int LPR>
__global__ __launch_bounds__(256) void rowsel_bucket_kernel(const BucketArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.rows) return;
    const int start = a.inv_ptr[row], end = a.inv_ptr[row + 1];
    for (int ch = lig; ch < a.chunks; ch += LPR) {
        const int64_t foff = (int64_t)ch * VEC;
        V P = V(0.f);
        for (int k = start; k < end; ++k) P += *(const V *)(a.G + (int64_t)a.inv_pos[k] * a.ldg + foff);
        *(V *)(a.out + row * a.ldout + foff) = P;
    }
}

template <int VEC>
int launch_bucket(BucketArgs a, hipStream_t st)
{
    a.chunks = (a.d + VEC - 1) / VEC;
    const int lpr = a.chunks <= 4 ? 4 : a.chunks <= 8 ? 8 : a.chunks <= 16 ? 16 : a.chunks <= 32 ? 32 : 64;
    const dim3 grid((unsigned)((a.rows + 256 / lpr - 1) / (256 / lpr)));
    switch (lpr) {
    case 4: hipLaunchKernelGGL((rowsel_bucket_kernel<VEC, 4>), grid, dim3(256), 0, st, a); break;
    case 8: hipLaunchKernelGGL((rowsel_bucket_kernel<VEC, 8>), grid, dim3(256), 0, st, a); break;
    case 16: hipLaunchKernelGGL((rowsel_bucket_kernel<VEC, 16>), grid, dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL((rowsel_bucket_kernel<VEC, 32>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((rowsel_bucket_kernel<VEC, 64>), grid, dim3(256), 0, st, a); break;
    }
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

// ------------------------------------------------------------------------------------------------ weighted reconstruction loss
constexpr int WR_THREADS = 256;

struct WreconArgs {
    int64_t B, N;
    const float *Z;
    int64_t ldz;
    const int32_t *tgt;      // [B] stacked row ids, -1 an all-zero target
    const int64_t *ent_ptr;  // [B + 1]: where the entries of row b's target start in the staging area
    int64_t entries;         // ent_ptr[B]
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    float beta2;
    double beta2d;
    const float *div;        // per stacked row, or null
    double scale;
    int32_t relu;
    float *dZ;               // null: the loss alone
    int64_t lddz;
    double *row_loss;        // [B]
    float *staged;           // [entries]: z at the target's stored columns, read before the sweep may overwrite it
};

__device__ __forceinline__ double block_sum(double v, double *sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                                      // sm may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sm[0];
#pragma unroll
    for (int k = 1; k < WR_THREADS / 64; ++k) t += sm[k];
    return t;
}

// one workgroup per row of Z.  Thread t owns the columns 4 q .. 4 q + 3 of the quads q = t, t + 256, ... in the float4 and in the
// scalar form alike, so both add the same numbers in the same order.
template <int VEC>
__global__ __launch_bounds__(WR_THREADS) void wrecon_row_kernel(const WreconArgs a)
{
    __shared__ double sm[WR_THREADS / 64];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const float *z = a.Z + b * a.ldz;
    float *g = a.dZ ? a.dZ + b * a.lddz : nullptr;
    const int r = a.tgt[b];
    int start = 0, len = 0;
    if (r >= 0) {
        start = a.row_ptr[r];
        len = a.row_ptr[r + 1] - start;
    }
    const int64_t c0 = a.ent_ptr[b];
    const bool ok = c0 >= 0 && a.ent_ptr[b + 1] - c0 == len && c0 + len <= a.entries;    // else the row's loss is NaN
    float *zc = a.staged + (ok ? c0 : 0);
    if (ok)
        for (int k = t; k < len; k += WR_THREADS) zc[k] = z[a.col[start + k]];             // read back by the same thread below
    __syncthreads();                                                                       // dZ may be Z: every read of z[col] precedes the sweep

    const float div = a.div ? (r >= 0 ? a.div[r] : 0.f) : 1.f;
    const float gc = (float)(2.0 * a.scale / (double)div);
    double dense = 0.0;
    const int64_t quads = (a.N + 3) / 4;
    for (int64_t q = t; q < quads; q += WR_THREADS) {
        float s = 0.f;
        if (VEC == 4) {
            f4 x = *(const f4 *)(z + 4 * q);
            if (a.relu) x = relu_of(x);
            s = fmaf(x.x, x.x, s); s = fmaf(x.y, x.y, s); s = fmaf(x.z, x.z, s); s = fmaf(x.w, x.w, s);
            if (g) *(f4 *)(g + 4 * q) = x * gc;
        } else {
            for (int u = 0; u < 4; ++u) {
                const int64_t j = 4 * q + u;
                if (j < a.N) {
                    float x = z[j];
                    if (a.relu) x = fmaxf(x, 0.f);
                    s = fmaf(x, x, s);
                    if (g) g[j] = x * gc;
                }
            }
        }
        dense += (double)s;
    }
    __syncthreads();                                                                       // the sweep's stores precede the corrected ones

    double corr = 0.0;
    if (ok)
        for (int k = t; k < len; k += WR_THREADS) {
            const float v = a.val[start + k];
            if (v == 0.f) continue;                                                        // a stored zero is no entry (the reference's x != 0)
            const float zz = zc[k];
            const float p = a.relu ? fmaxf(zz, 0.f) : zz;
            const double dd = (double)p - (double)v;
            corr += a.beta2d * dd * dd - (double)p * (double)p;
            if (g) g[a.col[start + k]] = (a.relu && !(zz > 0.f)) ? 0.f : gc * (a.beta2 * (p - v));
        }
    dense = block_sum(dense, sm);
    corr = block_sum(corr, sm);
    if (t == 0) a.row_loss[b] = ok ? (dense + corr) / (double)div : __longlong_as_double(0x7ff8000000000000LL);
}

// loss = scale sum_b row_loss[b]: 256 runs of consecutive rows, each in row order, then the runs in run order
__global__ __launch_bounds__(WR_THREADS) void wrecon_final_kernel(int64_t B, const double *row_loss, double scale, float *loss)
{
    __shared__ double sm[WR_THREADS];
    const int64_t per = (B + WR_THREADS - 1) / WR_THREADS;
    const int64_t lo = min(B, threadIdx.x * per), hi = min(B, lo + per);
    double t = 0.0;
    for (int64_t b = lo; b < hi; ++b) t += row_loss[b];
    sm[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < WR_THREADS; ++k) t += sm[k];
        loss[0] = (float)(scale * t);
    }
}

size_t wrecon_row_bytes(int64_t B) { return ((size_t)B * sizeof(double) + 15) & ~(size_t)15; }

}  // namespace

extern "C" int32_t ctgcn_rowsel_max_slots(void) { return MAX_SLOTS; }

extern "C" int ctgcn_rowsel_conv_fwd_f32(int64_t n, int32_t slots, int32_t d, const int32_t *idx, const int32_t *row_ptr, const int32_t *col,
                                         const float *val, const float *S, int64_t lds, int64_t col_stride, const float *bias, int32_t epi,
                                         float *Y, int64_t ldy, const int32_t *long_pos, int32_t n_long, int32_t long_threshold,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "rowsel_conv_fwd";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (slots < 1 || slots > MAX_SLOTS) return ctgcn_fail(CTGCN_E_INVALID, what, "slots outside [1, ctgcn_rowsel_max_slots()]");
    if (epi != 0 && epi != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none) or 1 (ReLU)");
    if (col_stride < 0) return ctgcn_fail(CTGCN_E_INVALID, what, "negative col_stride");
    if (lds < d || ldy < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!idx || !row_ptr || !col || !val || !S || !Y) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    RowselArgs a{};
    a.n = n; a.d = d; a.slots = slots; a.idx = idx; a.row_ptr = row_ptr; a.col = col; a.val = val;
    a.src = S; a.ldsrc = lds; a.col_stride = col_stride; a.bias = bias; a.relu = epi; a.out = Y; a.ldout = ldy;
    a.part_ld = (d + 3) & ~3;
    if (int rc = set_long_rows(a, what, long_pos, n_long, long_threshold, a.part_ld, workspace, workspace_bytes,
                               "long positions need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (one piece per position)"))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    return float4_rows(d, {{S, lds}, {Y, ldy}, {bias, 0}}) ? launch_rowsel<4>(a, st) : launch_rowsel<1>(a, st);
}

extern "C" int ctgcn_rowsel_bucket_f32(int64_t rows, int32_t d, const int32_t *inv_ptr, const int32_t *inv_pos, const float *G, int64_t ldg,
                                       float *out, int64_t ldout, void *stream)
{
    const char *what = "rowsel_bucket";
    if (rows < 0 || rows > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= rows < 2^31 and d >= 1");
    if (ldg < d || ldout < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (rows == 0) return CTGCN_OK;
    if (!inv_ptr || !inv_pos || !G || !out) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    BucketArgs a{};
    a.rows = rows; a.d = d; a.inv_ptr = inv_ptr; a.inv_pos = inv_pos; a.G = G; a.ldg = ldg; a.out = out; a.ldout = ldout;
    hipStream_t st = (hipStream_t)stream;
    return float4_rows(d, {{G, ldg}, {out, ldout}}) ? launch_bucket<4>(a, st) : launch_bucket<1>(a, st);
}

extern "C" size_t ctgcn_wrecon_loss_workspace_bytes(int64_t n, int64_t entries)
{
    if (n < 0 || entries < 0) return 0;
    return wrecon_row_bytes(n) + (size_t)entries * sizeof(float);
}

extern "C" int ctgcn_wrecon_loss_f32(int64_t n, int64_t width, const float *Z, int64_t ldz, const int32_t *tgt, const int64_t *ent_ptr,
                                     int64_t entries, const int32_t *row_ptr, const int32_t *col, const float *val, double beta,
                                     const float *div, double scale, int32_t relu, float *dZ, int64_t lddz, float *loss, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    const char *what = "wrecon_loss";
    if (n < 0 || n > INT32_MAX || width < 1 || width > INT32_MAX) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and 1 <= width < 2^31");
    if (entries < 0) return ctgcn_fail(CTGCN_E_INVALID, what, "negative entry count");
    if (relu != 0 && relu != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "relu must be 0 or 1");
    if (ldz < width || (dZ && lddz < width)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below width");
    if (!loss) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        CTGCN_TRY(hipMemsetAsync(loss, 0, sizeof(float), st));
        return CTGCN_OK;
    }
    if (!Z || !tgt || !ent_ptr || !row_ptr || (entries > 0 && (!col || !val))) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < ctgcn_wrecon_loss_workspace_bytes(n, entries))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 16-byte aligned and hold ctgcn_wrecon_loss_workspace_bytes() bytes");
    WreconArgs a{};
    a.B = n; a.N = width; a.Z = Z; a.ldz = ldz; a.tgt = tgt; a.ent_ptr = ent_ptr; a.entries = entries; a.row_ptr = row_ptr; a.col = col; a.val = val;
    a.beta2d = beta * beta; a.beta2 = (float)a.beta2d; a.div = div; a.scale = scale; a.relu = relu; a.dZ = dZ; a.lddz = lddz;
    a.row_loss = (double *)workspace;
    a.staged = (float *)((char *)workspace + wrecon_row_bytes(n));
    // the float4 form needs whole quads; the row sums do not depend on the form
    const bool v4 = width % 4 == 0 && float4_rows(4, {{Z, ldz}, {dZ, lddz}});
    if (v4) hipLaunchKernelGGL(wrecon_row_kernel<4>, dim3((unsigned)n), dim3(WR_THREADS), 0, st, a);
    else hipLaunchKernelGGL(wrecon_row_kernel<1>, dim3((unsigned)n), dim3(WR_THREADS), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(wrecon_final_kernel, dim3(1), dim3(WR_THREADS), 0, st, n, (const double *)a.row_loss, scale, loss);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
