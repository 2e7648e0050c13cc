// ctgcn_gcn.hip — the GCN step of the EvolveGCN baseline (reference baseline/egcn.py:74, helper.py:27-47) on the GPU.
//
//   normalise   val_out = D^-1/2 A D^-1/2 (or D^-1 A) over a CSR that already holds the diagonal: row sums and the scale r_i in fp64, the
//               product r_i a_ij r_j in fp64, rounded to fp32 once — the reference's float64 scipy arithmetic followed by .float().
//   forward     Y[i] = act(sum_e val[e] S[col[e]]), optionally scores[i] = Y[i] · p for the next layer's top-k.
//   backward    dS[i] = sum_e val[e] (dY[col[e]] ∘ m(Y[col[e]])) over the same (symmetric) CSR; the mask is formed on the gathered row.
//
// Pull form: a group of LPR lanes owns a destination row and a float4 (or a float) per lane of it, the row's entries are read LPR at a
// time and handed round by shuffles, four gathered rows in flight per group.  Rows longer than long_threshold entries are left to a
// block-per-piece kernel: a piece is at most 4 long_threshold entries, its eight lane groups sum interleaved entries and are added in
// group order, the pieces of a row are added in piece order by a last kernel that also finishes the row.  No atomics: every sum has a
// fixed order, so repeated launches are bit-identical.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "ctgcn_try.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr float RRELU_SLOPE = (float)((1.0 / 8.0 + 1.0 / 3.0) / 2.0);   // F.rrelu in eval mode: the mean of its default bounds
constexpr int PIECE_FACTOR = 4;        // entries of a long row's piece, in units of long_threshold
constexpr int PIECE_THREADS = 256;
constexpr int PIECE_LANES = 32;        // lanes across the feature row in the piece kernel
constexpr int PIECE_GROUPS = PIECE_THREADS / PIECE_LANES;
constexpr int U = 4;                   // gathered rows in flight per lane group

template <int VEC> struct vec_of;
template <> struct vec_of<4> { using type = f4; };
template <> struct vec_of<1> { using type = float; };

__device__ __forceinline__ f4 vfma(float a, f4 x, f4 acc) { return f4{fmaf(a, x.x, acc.x), fmaf(a, x.y, acc.y), fmaf(a, x.z, acc.z), fmaf(a, x.w, acc.w)}; }
__device__ __forceinline__ float vfma(float a, float x, float acc) { return fmaf(a, x, acc); }
__device__ __forceinline__ float rrelu1(float y) { return y >= 0.f ? y : y * RRELU_SLOPE; }
__device__ __forceinline__ f4 rrelu(f4 y) { return f4{rrelu1(y.x), rrelu1(y.y), rrelu1(y.z), rrelu1(y.w)}; }
__device__ __forceinline__ float rrelu(float y) { return rrelu1(y); }
// torch's leaky_relu backward: a pre-activation of exactly 0 takes the slope; sign(Y) = sign(pre-activation) as the slope is positive
__device__ __forceinline__ float mask1(float g, float y) { return y > 0.f ? g : g * RRELU_SLOPE; }
__device__ __forceinline__ f4 masked(f4 g, f4 y) { return f4{mask1(g.x, y.x), mask1(g.y, y.y), mask1(g.z, y.z), mask1(g.w, y.w)}; }
__device__ __forceinline__ float masked(float g, float y) { return mask1(g, y); }
__device__ __forceinline__ float vdot(f4 a, f4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float vdot(float a, float b) { return a * b; }

struct GcnArgs {
    int64_t n;
    int32_t d;
    const int32_t *row_ptr;
    const int32_t *col;
    const float *val;
    const float *src;       // forward: S; backward: dY
    int64_t ldsrc;
    const float *ymask;     // backward with act 1: Y (row stride ldmask); else null
    int64_t ldmask;
    float *out;             // forward: Y; backward: dS
    int64_t ldout;
    int32_t act;            // forward only: applied when a row is finished
    const float *score_vec;
    float *score_out;
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t chunks;         // ceil(d / VEC)
    int32_t max_pieces;     // pieces a long row may be cut into (what the workspace holds)
    int32_t part_ld;        // floats per partial vector: d rounded up to 4
    float *part;            // [n_long][max_pieces][part_ld]
};

__host__ __device__ __forceinline__ int pieces_of(int len, int long_thresh, int max_pieces)
{
    const int64_t piece = (int64_t)PIECE_FACTOR * long_thresh;
    const int64_t np = (len + piece - 1) / piece;
    return (int)(np < 1 ? 1 : (np > max_pieces ? max_pieces : np));
}

template <int VEC, bool BWD>
__device__ __forceinline__ typename vec_of<VEC>::type gather_row(const GcnArgs &a, int64_t c, int64_t foff)
{
    using V = typename vec_of<VEC>::type;
    V x = *(const V *)(a.src + c * a.ldsrc + foff);
    if (BWD && a.ymask) x = masked(x, *(const V *)(a.ymask + c * a.ldmask + foff));
    return x;
}

template <int VEC, int LPR, bool BWD>
__global__ __launch_bounds__(256) void gcn_row_kernel(const GcnArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    const int start = a.row_ptr[row], end = a.row_ptr[row + 1];
    if (a.n_long > 0 && end - start > a.long_thresh) return;      // long row: gcn_piece_kernel + gcn_final_kernel
    const bool score = !BWD && a.score_vec && a.score_out;
    float sc = 0.f;

    for (int p0 = 0; p0 < a.chunks; p0 += LPR) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        // dead lanes read chunk 0 (valid memory) and never store: keeps every load unconditional
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
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
                    xv[u] = gather_row<VEC, BWD>(a, cj, foff);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) P = vfma(wj[u], xv[u], P);
            }
            for (; j < cnt; ++j) {
                const int cj = __shfl(c, j, LPR);
                const float w1 = __shfl(w, j, LPR);
                P = vfma(w1, gather_row<VEC, BWD>(a, cj, foff), P);
            }
        }
        if (!BWD && a.act) P = rrelu(P);
        if (live) {
            *(V *)(a.out + row * a.ldout + foff) = P;
            if (score) sc += vdot(P, *(const V *)(a.score_vec + foff));
        }
    }
    if (score) {
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) sc += __shfl_xor(sc, o, LPR);
        if (lig == 0) a.score_out[row] = sc;
    }
}

// grid (max_pieces, n_long): block (p, i) sums piece p of long row i into part[i][p]
template <int VEC, bool BWD>
__global__ __launch_bounds__(PIECE_THREADS) void gcn_piece_kernel(const GcnArgs a)
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
        const int64_t foff = live ? (int64_t)ch * VEC : 0;
        V P = V(0.f);
        for (int e = lo + g; e < hi; e += PIECE_GROUPS) P = vfma(a.val[e], gather_row<VEC, BWD>(a, a.col[e], foff), P);
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

// one wave per long row: the pieces in piece order, the activation, the row and its score
template <bool BWD>
__global__ __launch_bounds__(64) void gcn_final_kernel(const GcnArgs a)
{
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const float *src = a.part + (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    const bool score = !BWD && a.score_vec && a.score_out;
    float sc = 0.f;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        float t = src[c];
        for (int p = 1; p < np; ++p) t += src[(int64_t)p * a.part_ld + c];
        if (!BWD && a.act) t = rrelu1(t);
        a.out[row * a.ldout + c] = t;
        if (score) sc = fmaf(t, a.score_vec[c], sc);
    }
    if (score) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
        if (threadIdx.x == 0) a.score_out[row] = sc;
    }
}

int fail(int code, const char *what, const char *text)
{
    char buf[192];
    snprintf(buf, sizeof(buf), "%s: %s", what, text);
    return ctgcn_set_error_(code, buf);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int VEC, int LPR, bool BWD>
void launch_rows(const GcnArgs &a, hipStream_t st)
{
    const int64_t rows_per_block = 256 / LPR;
    hipLaunchKernelGGL((gcn_row_kernel<VEC, LPR, BWD>), dim3((unsigned)((a.n + rows_per_block - 1) / rows_per_block)), dim3(256), 0, st, a);
}

template <int VEC, bool BWD>
int launch(GcnArgs a, hipStream_t st)
{
    a.chunks = (a.d + VEC - 1) / VEC;
    if (a.chunks <= 4) launch_rows<VEC, 4, BWD>(a, st);
    else if (a.chunks <= 8) launch_rows<VEC, 8, BWD>(a, st);
    else if (a.chunks <= 16) launch_rows<VEC, 16, BWD>(a, st);
    else if (a.chunks <= 32) launch_rows<VEC, 32, BWD>(a, st);
    else launch_rows<VEC, 64, BWD>(a, st);
    CTGCN_TRY(hipGetLastError());
    if (a.n_long > 0) {
        hipLaunchKernelGGL((gcn_piece_kernel<VEC, BWD>), dim3((unsigned)a.max_pieces, (unsigned)a.n_long), dim3(PIECE_THREADS), 0, st, a);
        CTGCN_TRY(hipGetLastError());
        hipLaunchKernelGGL((gcn_final_kernel<BWD>), dim3((unsigned)a.n_long), dim3(64), 0, st, a);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

// checks shared by the two layer entry points; fills the long-row fields
int set_common(GcnArgs &a, const char *what, int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val,
               const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes)
{
    if (n < 0 || n > INT32_MAX || d < 1) return fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (n_long < 0 || n_long > n) return fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val) return fail(CTGCN_E_INVALID, what, "null pointer");
    a.n = n; a.d = d; a.row_ptr = row_ptr; a.col = col; a.val = val;
    a.long_rows = long_rows; a.n_long = n_long; a.long_thresh = long_threshold;
    a.part_ld = (d + 3) & ~3;
    if (n_long > 0) {
        if (!long_rows) return fail(CTGCN_E_INVALID, what, "n_long > 0 without long_rows");
        if (long_threshold < 1 || long_threshold > INT32_MAX / PIECE_FACTOR) return fail(CTGCN_E_INVALID, what, "long_threshold outside [1, 2^29)");
        if (n_long > 65535) return fail(CTGCN_E_UNSUPPORTED, what, "more than 65535 long rows: raise long_threshold");
        const size_t one = (size_t)n_long * a.part_ld * sizeof(float);
        if (!workspace || !aligned16(workspace) || workspace_bytes < one)
            return fail(CTGCN_E_WORKSPACE, what, "long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (one piece per row)");
        const size_t mp = workspace_bytes / one;
        a.max_pieces = (int32_t)(mp > 4096 ? 4096 : mp);
        a.part = (float *)workspace;
    }
    return CTGCN_OK;
}

// ------------------------------------------------------------------------------------------------ normalisation
constexpr int NORM_LANES = 16;

__global__ __launch_bounds__(256) void gcn_rowscale_kernel(int64_t n, const int32_t *__restrict__ row_ptr, const float *__restrict__ val,
                                                           int row_norm, double *__restrict__ r, int32_t *flag)
{
    const int lig = threadIdx.x & (NORM_LANES - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;
    if (row >= n) return;
    double s = 0.0;
    for (int e = row_ptr[row] + lig, end = row_ptr[row + 1]; e < end; e += NORM_LANES) s += (double)val[e];
#pragma unroll
    for (int o = NORM_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, NORM_LANES);
    if (lig) return;
    if (s < 0.0) *flag = 1;                       // every writer stores the same value
    r[row] = s == 0.0 ? 0.0 : (row_norm ? 1.0 / s : 1.0 / sqrt(s));
}

__global__ __launch_bounds__(256) void gcn_scale_kernel(int64_t n, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ val, int row_norm, const double *__restrict__ r,
                                                        float *__restrict__ out)
{
    const int lig = threadIdx.x & (NORM_LANES - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;
    if (row >= n) return;
    const double ri = r[row];
    for (int e = row_ptr[row] + lig, end = row_ptr[row + 1]; e < end; e += NORM_LANES) {
        const double v = ri * (double)val[e];
        out[e] = (float)(row_norm ? v : v * r[col[e]]);
    }
}

}  // namespace

extern "C" size_t ctgcn_gcn_normalize_workspace_bytes(int64_t n) { return n < 0 ? 0 : (size_t)n * sizeof(double); }

extern "C" int ctgcn_gcn_normalize_f32(int64_t n, const int32_t *row_ptr, const int32_t *col, const float *val_in, int32_t row_norm,
                                       float *val_out, int32_t *flag, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_normalize";
    if (n < 0 || n > INT32_MAX) return fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31");
    if (row_norm != 0 && row_norm != 1) return fail(CTGCN_E_INVALID, what, "row_norm must be 0 or 1");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr || !col || !val_in || !val_out || !flag) return fail(CTGCN_E_INVALID, what, "null pointer");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < ctgcn_gcn_normalize_workspace_bytes(n))
        return fail(CTGCN_E_WORKSPACE, what, "workspace must be 8-byte aligned and hold ctgcn_gcn_normalize_workspace_bytes() bytes");
    hipStream_t st = (hipStream_t)stream;
    double *r = (double *)workspace;
    const unsigned grid = (unsigned)((n + 256 / NORM_LANES - 1) / (256 / NORM_LANES));
    CTGCN_TRY(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(gcn_rowscale_kernel, dim3(grid), dim3(256), 0, st, n, row_ptr, val_in, (int)row_norm, r, flag);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(gcn_scale_kernel, dim3(grid), dim3(256), 0, st, n, row_ptr, col, val_in, (int)row_norm, (const double *)r, val_out);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_gcn_layer_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                       int64_t lds, float *Y, int64_t ldy, int32_t act, const float *score_vec, float *score_out,
                                       const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_layer_fwd";
    GcnArgs a{};
    if (act != 0 && act != 1) return fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (eval-mode RReLU)");
    if (lds < d || ldy < d) return fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if ((score_vec == nullptr) != (score_out == nullptr)) return fail(CTGCN_E_INVALID, what, "score_vec and score_out go together");
    if (int rc = set_common(a, what, n, d, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!S || !Y) return fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = S; a.ldsrc = lds; a.out = Y; a.ldout = ldy; a.act = act; a.score_vec = score_vec; a.score_out = score_out;
    const bool v4 = d % 4 == 0 && lds % 4 == 0 && ldy % 4 == 0 && aligned16(S) && aligned16(Y) && (!score_vec || aligned16(score_vec));
    return v4 ? launch<4, false>(a, (hipStream_t)stream) : launch<1, false>(a, (hipStream_t)stream);
}

extern "C" int ctgcn_gcn_layer_bwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *dY,
                                       int64_t lddy, const float *Y, int64_t ldy, int32_t act, float *dS, int64_t ldds,
                                       const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "gcn_layer_bwd";
    GcnArgs a{};
    if (act != 0 && act != 1) return fail(CTGCN_E_INVALID, what, "act must be 0 (identity) or 1 (eval-mode RReLU)");
    if (lddy < d || ldds < d || (act && ldy < d)) return fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (int rc = set_common(a, what, n, d, row_ptr, col, val, long_rows, n_long, long_threshold, workspace, workspace_bytes)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!dY || !dS || (act && !Y)) return fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = dY; a.ldsrc = lddy; a.ymask = act ? Y : nullptr; a.ldmask = act ? ldy : 0; a.out = dS; a.ldout = ldds; a.act = act;
    const bool v4 = d % 4 == 0 && lddy % 4 == 0 && ldds % 4 == 0 && aligned16(dY) && aligned16(dS) && (!act || (ldy % 4 == 0 && aligned16(Y)));
    return v4 ? launch<4, true>(a, (hipStream_t)stream) : launch<1, true>(a, (hipStream_t)stream);
}
