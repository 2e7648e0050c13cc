// ctgcn_pool.hip — the pooling layers of the GIN and GraphSAGE baselines (reference baseline/gin.py, baseline/sage.py) on the GPU.
//
//   pool conv   Y[i] = epi(sum_e val[e] S[col[e]] + self_scale T[i] + b); epi none, or ReLU, the row's L2 normalisation and
//               counter-based dropout (ctgcn_rng.h).  One pass is a whole GraphSAGE layer after its product, or GIN's sum / average
//               pooling with a learnt eps.  Without a matrix (row_ptr null) it is the epilogue alone.
//   conv prep   the backward's one N x d pass: G = d loss / d (pre-epilogue sum) from dY, the normalised rows and their norms, the
//               dropout draw made again, and the bias gradient as per-block column sums added in block order.
//   pool max    Y[i, c] = max_e S[col[e], c] with arg[i, c] the winning column index (the lowest among equal values, -1 and 0 for an
//               empty row); the backward pulls over the transposed CSR: dS[j, c] = sum_i [arg[i, c] == j] dY[i, c], in ascending i.
//   batch norm  column statistics in fp64 (per-block shifted sums, merged by Chan's formula in a fixed order), the apply pass
//               y = dropout(relu((x - mean) rstd w + b)), and a backward that recomputes the ReLU mask and the draw from x.
//
// Pull form as in ctgcn_gather.h: a group of LPR lanes owns a destination row, each lane a float4 (or a float) of it, and walks the
// row's entries in order.  Rows longer than long_threshold entries go to a block-per-piece kernel (a piece is at most
// 4 long_threshold entries; its eight lane groups take interleaved entries and are combined in group order) and a last kernel that
// combines the pieces in piece order and finishes the row.  No atomics: every sum has a fixed order, and the maximum breaks ties by
// the column index, so repeated launches are bit-identical.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

typedef int i4 __attribute__((ext_vector_type(4)));

constexpr int MODE_SUM = 0, MODE_MAX = 1, MODE_PULL = 2;

template <int VEC> __device__ __forceinline__ void ldf(const float *p, float (&x)[VEC]);
template <> __device__ __forceinline__ void ldf<4>(const float *p, float (&x)[4])
{
    const f4 t = *(const f4 *)p;
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
}
template <> __device__ __forceinline__ void ldf<1>(const float *p, float (&x)[1]) { x[0] = *p; }
template <int VEC> __device__ __forceinline__ void stf(float *p, const float (&x)[VEC]);
template <> __device__ __forceinline__ void stf<4>(float *p, const float (&x)[4]) { *(f4 *)p = f4{x[0], x[1], x[2], x[3]}; }
template <> __device__ __forceinline__ void stf<1>(float *p, const float (&x)[1]) { *p = x[0]; }
template <int VEC> __device__ __forceinline__ void ldi(const int32_t *p, int (&x)[VEC]);
template <> __device__ __forceinline__ void ldi<4>(const int32_t *p, int (&x)[4])
{
    const i4 t = *(const i4 *)p;
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
}
template <> __device__ __forceinline__ void ldi<1>(const int32_t *p, int (&x)[1]) { x[0] = *p; }
template <int VEC> __device__ __forceinline__ void sti(int32_t *p, const int (&x)[VEC]);
template <> __device__ __forceinline__ void sti<4>(int32_t *p, const int (&x)[4]) { *(i4 *)p = i4{x[0], x[1], x[2], x[3]}; }
template <> __device__ __forceinline__ void sti<1>(int32_t *p, const int (&x)[1]) { *p = x[0]; }

struct PoolArgs {
    int64_t n;
    int32_t d, chunks;
    const int32_t *row_ptr; // null: no matrix, every row is empty (the epilogue alone)
    const int32_t *col;
    const float *val;       // SUM only
    const float *src;       // SUM, MAX: S; PULL: dY
    int64_t ldsrc;
    const int32_t *argin;   // PULL: the forward's arg
    int64_t ldargin;
    const float *self;      // SUM: T or null
    int64_t ldself;
    float self_scale;
    const float *bias;      // SUM: [d] or null
    float *out;             // SUM, MAX: Y; PULL: dS
    int64_t ldout;
    int32_t *argout;        // MAX
    int64_t ldargout;
    int32_t epi, drop;      // SUM: epi 1 = ReLU, L2 row normalisation, dropout when drop
    float *norm;            // [n]: the norm of the ReLU'd row before the clamp
    float *ysave;           // with drop: the normalised row before dropout, for the backward
    int64_t ldsave;
    double p;
    float scale;            // 1 / (1 - p)
    uint64_t key;
    const int32_t *long_rows;
    int32_t n_long, long_thresh;
    int32_t max_pieces;     // pieces a long row may be cut into (what the workspace holds)
    int32_t part_ld;        // floats per partial vector: d rounded up to 4
    float *part;            // [n_long][max_pieces][part_ld]
    int32_t *part_arg;      // MAX: the same shape
};

// the candidate (x, c) against the best so far: larger wins, the lower column index among equals; c < 0 is no candidate
__device__ __forceinline__ void better(float x, int c, float &best, int &arg)
{
    if (c < 0) return;
    if (arg < 0 || x > best || (x == best && c < arg)) {
        best = x;
        arg = c;
    }
}

// the entries lo, lo + step, ... below hi of a row into acc (and arg): the weighted sum, the maximum, or the backward's masked sum
template <int VEC, int MODE>
__device__ __forceinline__ void accumulate(const PoolArgs &a, int64_t row, int lo, int hi, int step, int64_t foff, float (&acc)[VEC], int (&arg)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        acc[k] = 0.f;
        arg[k] = -1;
    }
#pragma unroll 4
    for (int e = lo; e < hi; e += step) {
        const int c = a.col[e];
        float x[VEC];
        ldf<VEC>(a.src + (int64_t)c * a.ldsrc + foff, x);
        if (MODE == MODE_SUM) {
            const float w = a.val[e];
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] = fmaf(w, x[k], acc[k]);
        } else if (MODE == MODE_MAX) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) better(x[k], c, acc[k], arg[k]);
        } else {
            int ai[VEC];
            ldi<VEC>(a.argin + (int64_t)c * a.ldargin + foff, ai);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += ai[k] == (int)row ? x[k] : 0.f;
        }
    }
}

// SUM: the self term and the bias onto a finished sum; without epilogue the row is done, with it the ReLU'd values are stored and
// their squares returned
template <int VEC>
__device__ __forceinline__ float finish_sum(const PoolArgs &a, int64_t row, int64_t foff, float (&acc)[VEC])
{
    if (a.self) {
        float t[VEC];
        ldf<VEC>(a.self + row * a.ldself + foff, t);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = fmaf(a.self_scale, t[k], acc[k]);
    }
    if (a.bias) {
        float b[VEC];
        ldf<VEC>(a.bias + foff, b);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += b[k];
    }
    float ss = 0.f;
    if (a.epi) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            acc[k] = acc[k] > 0.f ? acc[k] : 0.f;
            ss = fmaf(acc[k], acc[k], ss);
        }
    }
    stf<VEC>(a.out + row * a.ldout + foff, acc);
    return ss;
}

// the epilogue's second half on values this thread stored itself: the division by the clamped norm, then dropout
template <int VEC>
__device__ __forceinline__ void rescale(const PoolArgs &a, int64_t row, int64_t foff, float den)
{
    float y[VEC];
    ldf<VEC>(a.out + row * a.ldout + foff, y);
#pragma unroll
    for (int k = 0; k < VEC; ++k) y[k] = y[k] / den;
    if (a.drop) {
        if (a.ysave) stf<VEC>(a.ysave + row * a.ldsave + foff, y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) y[k] = ctgcn_u01(a.key, (uint64_t)row, (uint64_t)(foff + k)) >= a.p ? y[k] * a.scale : 0.f;
    }
    stf<VEC>(a.out + row * a.ldout + foff, y);
}

// every row that is not long
template <int VEC, int LPR, int MODE>
__global__ __launch_bounds__(256) void pool_row_kernel(const PoolArgs a)
{
    const int lig = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= a.n) return;
    int start = 0, end = 0;
    if (a.row_ptr) {
        start = a.row_ptr[row];
        end = a.row_ptr[row + 1];
    }
    if (a.n_long > 0 && end - start > a.long_thresh) return;      // long row: pool_piece_kernel + pool_final_kernel
    float ss = 0.f;
    for (int ch = lig; ch < a.chunks; ch += LPR) {
        const int64_t foff = (int64_t)ch * VEC;
        float acc[VEC];
        int arg[VEC];
        accumulate<VEC, MODE>(a, row, start, end, 1, foff, acc, arg);
        if (MODE == MODE_SUM) {
            ss += finish_sum<VEC>(a, row, foff, acc);
        } else {
            stf<VEC>(a.out + row * a.ldout + foff, acc);
            if (MODE == MODE_MAX) sti<VEC>(a.argout + row * a.ldargout + foff, arg);
        }
    }
    if (MODE != MODE_SUM || !a.epi) return;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, LPR);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, L2_EPS);
    if (lig == 0) a.norm[row] = nrm;
    for (int ch = lig; ch < a.chunks; ch += LPR) rescale<VEC>(a, row, (int64_t)ch * VEC, den);
}

// grid (max_pieces, n_long): block (p, i) combines piece p of long row i into part[i][p]
template <int VEC, int MODE>
__global__ __launch_bounds__(PIECE_THREADS) void pool_piece_kernel(const PoolArgs a)
{
    __shared__ float smv[PIECE_GROUPS][PIECE_LANES * VEC];
    __shared__ int sma[PIECE_GROUPS][PIECE_LANES * VEC];
    const int64_t row = a.long_rows[blockIdx.y];
    const int start = a.row_ptr[row], len = a.row_ptr[row + 1] - start;
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const int p = blockIdx.x;
    if (p >= np) return;
    const int plen = (len + np - 1) / np;
    const int lo = start + min(len, p * plen), hi = start + min(len, (p + 1) * plen);
    const int lig = threadIdx.x & (PIECE_LANES - 1), g = threadIdx.x / PIECE_LANES;
    const int64_t dst = ((int64_t)blockIdx.y * a.max_pieces + p) * a.part_ld;

    for (int p0 = 0; p0 < a.chunks; p0 += PIECE_LANES) {
        const int ch = p0 + lig;
        const bool live = ch < a.chunks;
        const int64_t foff = live ? (int64_t)ch * VEC : 0;        // dead lanes read chunk 0 (valid memory) and never store
        float acc[VEC];
        int arg[VEC];
        accumulate<VEC, MODE>(a, row, lo + g, hi, PIECE_GROUPS, foff, acc, arg);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            smv[g][lig * VEC + k] = acc[k];
            sma[g][lig * VEC + k] = arg[k];
        }
        __syncthreads();
        if (g == 0 && live) {
            for (int q = 1; q < PIECE_GROUPS; ++q) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    if (MODE == MODE_MAX) better(smv[q][lig * VEC + k], sma[q][lig * VEC + k], acc[k], arg[k]);
                    else acc[k] += smv[q][lig * VEC + k];
                }
            }
            stf<VEC>(a.part + dst + foff, acc);
            if (MODE == MODE_MAX) sti<VEC>(a.part_arg + dst + foff, arg);
        }
        __syncthreads();
    }
}

// one wave per long row: the pieces in piece order, then what the row kernel does with a finished row
template <int MODE>
__global__ __launch_bounds__(64) void pool_final_kernel(const PoolArgs a)
{
    const int64_t row = a.long_rows[blockIdx.x];
    const int len = a.row_ptr[row + 1] - a.row_ptr[row];
    const int np = pieces_of(len, a.long_thresh, a.max_pieces);
    const int64_t base = (int64_t)blockIdx.x * a.max_pieces * a.part_ld;
    float ss = 0.f;
    for (int c = threadIdx.x; c < a.d; c += 64) {
        float t[1] = {a.part[base + c]};
        int g = MODE == MODE_MAX ? a.part_arg[base + c] : 0;
        for (int p = 1; p < np; ++p) {
            const int64_t at = base + (int64_t)p * a.part_ld + c;
            if (MODE == MODE_MAX) better(a.part[at], a.part_arg[at], t[0], g);
            else t[0] += a.part[at];
        }
        if (MODE == MODE_SUM) {
            ss += finish_sum<1>(a, row, c, t);
        } else {
            a.out[row * a.ldout + c] = t[0];
            if (MODE == MODE_MAX) a.argout[row * a.ldargout + c] = g;
        }
    }
    if (MODE != MODE_SUM || !a.epi) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float nrm = sqrtf(ss);
    const float den = fmaxf(nrm, L2_EPS);
    if (threadIdx.x == 0) a.norm[row] = nrm;
    for (int c = threadIdx.x; c < a.d; c += 64) rescale<1>(a, row, c, den);
}

// ------------------------------------------------------------------------------------------------ pool conv: backward pre-pass
// PREP_ROWS rows a block, one partial column-sum vector per block; colsum_kernel (ctgcn_gather.h) adds them in block order
struct PrepArgs {
    int64_t n;
    int32_t d, chunks, drop;
    const float *dY;
    int64_t lddy;
    const float *Y;         // the normalised rows before dropout
    int64_t ldy;
    const float *norm;
    double p;
    float scale;
    uint64_t key;
    float *G;
    int64_t ldg;
    float *part;            // [blocks][part_ld] or null
    int32_t part_ld;
};

// dY through the dropout draw, made again from the key
template <int VEC>
__device__ __forceinline__ void undrop(const PrepArgs &a, int64_t r, int64_t foff, float (&g)[VEC])
{
    if (!a.drop) return;
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k] = ctgcn_u01(a.key, (uint64_t)r, (uint64_t)(foff + k)) >= a.p ? g[k] * a.scale : 0.f;
}

template <int VEC>
__global__ __launch_bounds__(64 * PREP_WAVES) void pool_prep_kernel(const PrepArgs a)
{
    __shared__ float sm[PREP_WAVES][64 * VEC];
    __shared__ float s_dot[PREP_ROWS], s_den[PREP_ROWS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;

    for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
        const int64_t r = row0 + k;
        float dot = 0.f;
        for (int ch = lane; ch < a.chunks; ch += 64) {
            const int64_t foff = (int64_t)ch * VEC;
            float y[VEC], g[VEC];
            ldf<VEC>(a.Y + r * a.ldy + foff, y);
            ldf<VEC>(a.dY + r * a.lddy + foff, g);
            undrop<VEC>(a, r, foff, g);
#pragma unroll
            for (int q = 0; q < VEC; ++q) dot = fmaf(y[q], g[q], dot);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        if (lane == 0) {
            const float nrm = a.norm[r];
            const bool ok = nrm >= L2_EPS;                        // below the clamp the denominator was the constant eps
            s_dot[k] = ok ? dot : 0.f;
            s_den[k] = ok ? nrm : L2_EPS;
        }
    }
    __syncthreads();
    for (int p0 = 0; p0 < a.chunks; p0 += 64) {
        const int ch = p0 + lane;
        const bool live = ch < a.chunks;
        const int64_t foff = (int64_t)ch * VEC;
        float acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
        if (live) {
            for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
                const int64_t r = row0 + k;
                float y[VEC], g[VEC];
                ldf<VEC>(a.Y + r * a.ldy + foff, y);
                ldf<VEC>(a.dY + r * a.lddy + foff, g);
                undrop<VEC>(a, r, foff, g);
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    g[q] = y[q] > 0.f ? (g[q] - y[q] * s_dot[k]) / s_den[k] : 0.f;     // the ReLU passed exactly where the row is positive
                    acc[q] += g[q];
                }
                stf<VEC>(a.G + r * a.ldg + foff, g);
            }
        }
        if (a.part) {                                             // block-uniform
#pragma unroll
            for (int q = 0; q < VEC; ++q) sm[w][lane * VEC + q] = acc[q];
            __syncthreads();
            if (w == 0 && live) {
                for (int k = 1; k < PREP_WAVES; ++k)
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] += sm[k][lane * VEC + q];
                stf<VEC>(a.part + (int64_t)blockIdx.x * a.part_ld + foff, acc);
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ column batch norm
constexpr int BN_ROWS = 128;           // rows of a statistics block: one (mean, M2) pair per block and column
constexpr int BN_COLS = 64;

// grid (ceil(d / 64), ceil(n / 128)): wave w takes the block's rows w, w + 4, ...; sums of x - K and (x - K)^2 in fp64 with K the
// block's first row, so the squares stay small beside a large mean; part[b][c] = {block mean, block M2}
__global__ __launch_bounds__(BN_COLS * 4) void bn_stats_kernel(int64_t n, int32_t d, const float *x, int64_t ldx, double *part)
{
    __shared__ double s1[4][BN_COLS], s2[4][BN_COLS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * BN_COLS + lane;
    const int64_t row0 = (int64_t)blockIdx.y * BN_ROWS;
    const int64_t rows = min((int64_t)BN_ROWS, n - row0);
    double a1 = 0.0, a2 = 0.0, K = 0.0;
    if (c < d) {
        K = (double)x[row0 * ldx + c];
        for (int64_t k = w; k < rows; k += 4) {
            const double t = (double)x[(row0 + k) * ldx + c] - K;
            a1 += t;
            a2 = fma(t, t, a2);
        }
    }
    s1[w][lane] = a1;
    s2[w][lane] = a2;
    __syncthreads();
    if (w == 0 && c < d) {
        for (int k = 1; k < 4; ++k) {
            a1 += s1[k][lane];
            a2 += s2[k][lane];
        }
        double *dst = part + ((int64_t)blockIdx.y * d + c) * 2;
        dst[0] = K + a1 / (double)rows;
        dst[1] = a2 - a1 * a1 / (double)rows;
    }
}

// Chan's merge of (count, mean, M2) pairs
__device__ __forceinline__ void chan(double &na, double &ma, double &qa, double nb, double mb, double qb)
{
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb; ma = mb; qa = qb;
        return;
    }
    const double nn = na + nb, dl = mb - ma;
    ma += dl * (nb / nn);
    qa += qb + dl * dl * (na * nb / nn);
    na = nn;
}

// the blocks of a column merged as DB_SEGS runs of consecutive blocks, each in block order, then the runs in run order
__global__ __launch_bounds__(DB_COLS * DB_SEGS) void bn_merge_kernel(int64_t n, int64_t blocks, int32_t d, const double *part, double eps, float *mean,
                                                                     float *var, float *rstd)
{
    __shared__ double sn[DB_SEGS][DB_COLS], sm[DB_SEGS][DB_COLS], sq[DB_SEGS][DB_COLS];
    const int cx = threadIdx.x % DB_COLS, seg = threadIdx.x / DB_COLS;
    const int64_t c = (int64_t)blockIdx.x * DB_COLS + cx;
    const int64_t per = (blocks + DB_SEGS - 1) / DB_SEGS;
    const int64_t lo = min(blocks, seg * per), hi = min(blocks, lo + per);
    double na = 0.0, ma = 0.0, qa = 0.0;
    if (c < d)
        for (int64_t b = lo; b < hi; ++b) {
            const double *src = part + (b * d + c) * 2;
            chan(na, ma, qa, (double)min((int64_t)BN_ROWS, n - b * BN_ROWS), src[0], src[1]);
        }
    sn[seg][cx] = na;
    sm[seg][cx] = ma;
    sq[seg][cx] = qa;
    __syncthreads();
    if (seg == 0 && c < d) {
        for (int k = 1; k < DB_SEGS; ++k) chan(na, ma, qa, sn[k][cx], sm[k][cx], sq[k][cx]);
        const double v = qa > 0.0 ? qa / na : 0.0;
        mean[c] = (float)ma;
        var[c] = (float)v;
        rstd[c] = (float)(1.0 / sqrt(v + eps));
    }
}

struct BnArgs {
    int64_t n;
    int32_t d, chunks, relu, drop;
    const float *x;
    int64_t ldx;
    const float *mean, *rstd, *w, *b;
    double p;
    float scale;
    uint64_t key;
    float *y;               // apply
    int64_t ldy;
    const float *dy;        // backward
    int64_t lddy;
    float *dx;
    int64_t lddx;
    const float *dw, *db;   // the finished column sums, for the dx pass
    float inv_n;            // 1 / n with batch statistics, 0 with given ones (they do not depend on x)
    float *part;            // [2][blocks][part_ld]: the column sums of g and of g x_hat
    int32_t part_ld;
    int64_t blocks;
};

// x_hat and the value before the ReLU: one expression for the forward and for the backward's mask
__device__ __forceinline__ float bn_pre(float x, float mean, float rstd, float w, float b, float &xhat)
{
    xhat = (x - mean) * rstd;
    return fmaf(xhat, w, b);
}

// x_hat and g = dy through dropout and the ReLU, both made again from x
template <int VEC>
__device__ __forceinline__ void bn_grad(const BnArgs &a, int64_t r, int64_t foff, float (&xh)[VEC], float (&g)[VEC])
{
    float x[VEC], m[VEC], s[VEC], w[VEC], b[VEC];
    ldf<VEC>(a.x + r * a.ldx + foff, x);
    ldf<VEC>(a.dy + r * a.lddy + foff, g);
    ldf<VEC>(a.mean + foff, m);
    ldf<VEC>(a.rstd + foff, s);
    ldf<VEC>(a.w + foff, w);
    ldf<VEC>(a.b + foff, b);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float pre = bn_pre(x[k], m[k], s[k], w[k], b[k], xh[k]);
        if (a.relu && !(pre > 0.f)) g[k] = 0.f;
        else if (a.drop) g[k] = ctgcn_u01(a.key, (uint64_t)r, (uint64_t)(foff + k)) >= a.p ? g[k] * a.scale : 0.f;
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const BnArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n * a.chunks) return;
    const int64_t r = idx / a.chunks, foff = (idx % a.chunks) * VEC;
    float x[VEC], m[VEC], s[VEC], w[VEC], b[VEC];
    ldf<VEC>(a.x + r * a.ldx + foff, x);
    ldf<VEC>(a.mean + foff, m);
    ldf<VEC>(a.rstd + foff, s);
    ldf<VEC>(a.w + foff, w);
    ldf<VEC>(a.b + foff, b);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float xh;
        float v = bn_pre(x[k], m[k], s[k], w[k], b[k], xh);
        if (a.relu) v = v > 0.f ? v : 0.f;
        if (a.drop) v = ctgcn_u01(a.key, (uint64_t)r, (uint64_t)(foff + k)) >= a.p ? v * a.scale : 0.f;
        x[k] = v;
    }
    stf<VEC>(a.y + r * a.ldy + foff, x);
}

// per-block column sums of g (db) and g x_hat (dw), the layout of pool_prep_kernel
template <int VEC>
__global__ __launch_bounds__(64 * PREP_WAVES) void bn_bwd_reduce_kernel(const BnArgs a)
{
    __shared__ float smb[PREP_WAVES][64 * VEC], smw[PREP_WAVES][64 * VEC];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    for (int p0 = 0; p0 < a.chunks; p0 += 64) {
        const int ch = p0 + lane;
        const bool live = ch < a.chunks;
        const int64_t foff = (int64_t)ch * VEC;
        float ab[VEC], aw[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) ab[q] = aw[q] = 0.f;
        if (live) {
            for (int k = w; k < PREP_ROWS && row0 + k < a.n; k += PREP_WAVES) {
                float xh[VEC], g[VEC];
                bn_grad<VEC>(a, row0 + k, foff, xh, g);
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    ab[q] += g[q];
                    aw[q] = fmaf(g[q], xh[q], aw[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            smb[w][lane * VEC + q] = ab[q];
            smw[w][lane * VEC + q] = aw[q];
        }
        __syncthreads();
        if (w == 0 && live) {
            for (int k = 1; k < PREP_WAVES; ++k)
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    ab[q] += smb[k][lane * VEC + q];
                    aw[q] += smw[k][lane * VEC + q];
                }
            stf<VEC>(a.part + (int64_t)blockIdx.x * a.part_ld + foff, ab);
            stf<VEC>(a.part + (a.blocks + blockIdx.x) * a.part_ld + foff, aw);
        }
        __syncthreads();
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const BnArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n * a.chunks) return;
    const int64_t r = idx / a.chunks, foff = (idx % a.chunks) * VEC;
    float xh[VEC], g[VEC], s[VEC], w[VEC], dw[VEC], db[VEC];
    bn_grad<VEC>(a, r, foff, xh, g);
    ldf<VEC>(a.rstd + foff, s);
    ldf<VEC>(a.w + foff, w);
    ldf<VEC>(a.dw + foff, dw);
    ldf<VEC>(a.db + foff, db);
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k] = w[k] * s[k] * (g[k] - db[k] * a.inv_n - xh[k] * (dw[k] * a.inv_n));
    stf<VEC>(a.dx + r * a.lddx + foff, g);
}

// ------------------------------------------------------------------------------------------------ host side
template <int VEC, int MODE>
int launch(PoolArgs a, hipStream_t st)
{
    a.chunks = a.d / VEC;                                         // VEC 4 only when d % 4 == 0
    return launch_rows(
        a, [&](auto lpr, dim3 grid) { hipLaunchKernelGGL((pool_row_kernel<VEC, decltype(lpr)::value, MODE>), grid, dim3(256), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL((pool_piece_kernel<VEC, MODE>), grid, dim3(PIECE_THREADS), 0, st, a); },
        [&](dim3 grid) { hipLaunchKernelGGL(pool_final_kernel<MODE>, grid, dim3(64), 0, st, a); });
}

template <int MODE>
int dispatch(const PoolArgs &a, bool v4, void *stream)
{
    return v4 ? launch<4, MODE>(a, (hipStream_t)stream) : launch<1, MODE>(a, (hipStream_t)stream);
}

// checks shared by the three gather entry points; fills the matrix and long-row fields.  words: 4-byte words per partial element
// (1: a sum; 2: a maximum and its index)
int set_common(PoolArgs &a, const char *what, int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const int32_t *long_rows,
               int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, int words)
{
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (n_long < 0 || n_long > n) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long outside [0, n]");
    if (n == 0) return CTGCN_OK;
    if (!row_ptr && n_long > 0) return ctgcn_fail(CTGCN_E_INVALID, what, "long rows without a matrix");
    if (row_ptr && !col) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.n = n; a.d = d; a.row_ptr = row_ptr; a.col = col;
    a.part_ld = (d + 3) & ~3;
    if (int rc = set_long_rows(a, what, long_rows, n_long, long_threshold, (size_t)a.part_ld * words, workspace, workspace_bytes,
                               "long rows need a 16-byte aligned workspace of at least n_long * round_up(d, 4) * 4 bytes (8 for pool_max_fwd), one piece per row"))
        return rc;
    if (n_long > 0 && words == 2) a.part_arg = (int32_t *)workspace + (size_t)n_long * a.max_pieces * a.part_ld;
    return CTGCN_OK;
}

int64_t prep_blocks(int64_t n) { return (n + PREP_ROWS - 1) / PREP_ROWS; }

int check_bn(const char *what, int64_t n, int32_t d, const float *x, int64_t ldx, const float *mean, const float *rstd, const float *w,
             const float *b, int32_t relu, double p)
{
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (relu != 0 && relu != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "relu must be 0 or 1");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (n == 0) return CTGCN_OK;
    if (!x || !mean || !rstd || !w || !b) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (ldx < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    return CTGCN_OK;
}

void set_bn(BnArgs &a, int64_t n, int32_t d, const float *x, int64_t ldx, const float *mean, const float *rstd, const float *w, const float *b,
            int32_t relu, double p, uint64_t key)
{
    a.n = n; a.d = d; a.x = x; a.ldx = ldx; a.mean = mean; a.rstd = rstd; a.w = w; a.b = b;
    a.relu = relu; a.drop = p > 0.0; a.p = p; a.scale = 1.0f / (1.0f - (float)p); a.key = key;
}

}  // namespace

extern "C" int ctgcn_pool_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S,
                                       int64_t lds, const float *T, int64_t ldt, float self_scale, const float *bias, float *Y, int64_t ldy,
                                       int32_t epi, double p, uint64_t key, float *norm, float *Ysave, int64_t ldsave,
                                       const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    const char *what = "pool_conv_fwd";
    PoolArgs a{};
    if (epi != 0 && epi != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "epi must be 0 (none) or 1 (ReLU, L2 row normalisation, dropout)");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    const bool drop = epi == 1 && p > 0.0;
    if ((row_ptr && lds < d) || ldy < d || (T && ldt < d) || (drop && Ysave && ldsave < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (int rc = set_common(a, what, n, d, row_ptr, col, long_rows, n_long, long_threshold, workspace, workspace_bytes, 1)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!Y || (row_ptr && (!S || !val)) || (epi == 1 && !norm)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.val = val; a.src = S; a.ldsrc = lds; a.self = T; a.ldself = ldt; a.self_scale = self_scale; a.bias = bias; a.out = Y; a.ldout = ldy;
    a.epi = epi; a.drop = drop; a.norm = norm; a.ysave = drop ? Ysave : nullptr; a.ldsave = ldsave;
    a.p = p; a.scale = 1.0f / (1.0f - (float)p); a.key = key;
    return dispatch<MODE_SUM>(a, float4_rows(d, {{row_ptr ? S : nullptr, lds}, {T, ldt}, {Y, ldy}, {bias, 0}, {a.ysave, ldsave}}), stream);
}

extern "C" size_t ctgcn_pool_prep_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 0 || d < 1) return 0;
    return (size_t)prep_blocks(n) * (size_t)((d + 3) & ~3) * sizeof(float);
}

extern "C" int ctgcn_pool_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *norm,
                                        double p, uint64_t key, float *G, int64_t ldg, float *db, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    const char *what = "pool_conv_prep";
    if (n < 0 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= n < 2^31 and d >= 1");
    if (bad_p(p)) return ctgcn_fail(CTGCN_E_INVALID, what, "dropout p outside [0, 1)");
    if (n == 0) return CTGCN_OK;
    if (!dY || !Y || !G || !norm) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (lddy < d || ldy < d || ldg < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (db && (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < ctgcn_pool_prep_workspace_bytes(n, d)))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "a bias gradient needs a 16-byte aligned workspace of ctgcn_pool_prep_workspace_bytes() bytes");
    PrepArgs a{};
    a.n = n; a.d = d; a.drop = p > 0.0; a.dY = dY; a.lddy = lddy; a.Y = Y; a.ldy = ldy; a.norm = norm; a.p = p;
    a.scale = 1.0f / (1.0f - (float)p); a.key = key; a.G = G; a.ldg = ldg; a.part = db ? (float *)workspace : nullptr; a.part_ld = (d + 3) & ~3;
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = prep_blocks(n);
    const bool v4 = float4_rows(d, {{dY, lddy}, {Y, ldy}, {G, ldg}});
    a.chunks = v4 ? d / 4 : d;
    if (v4) hipLaunchKernelGGL(pool_prep_kernel<4>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    else hipLaunchKernelGGL(pool_prep_kernel<1>, dim3((unsigned)blocks), dim3(64 * PREP_WAVES), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    if (db) {
        hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), dim3((unsigned)((d + DB_COLS - 1) / DB_COLS)), dim3(DB_COLS * DB_SEGS), 0, st, blocks, d, a.part_ld,
                           (const float *)a.part, db);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

extern "C" int ctgcn_pool_max_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds, float *Y,
                                      int64_t ldy, int32_t *arg, int64_t ldarg, const int32_t *long_rows, int32_t n_long,
                                      int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "pool_max_fwd";
    PoolArgs a{};
    if (lds < d || ldy < d || ldarg < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n > 0 && !row_ptr) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (int rc = set_common(a, what, n, d, row_ptr, col, long_rows, n_long, long_threshold, workspace, workspace_bytes, 2)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!S || !Y || !arg) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = S; a.ldsrc = lds; a.out = Y; a.ldout = ldy; a.argout = arg; a.ldargout = ldarg;
    return dispatch<MODE_MAX>(a, float4_rows(d, {{S, lds}, {Y, ldy}, {arg, ldarg}}), stream);
}

extern "C" int ctgcn_pool_max_bwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *dY, int64_t lddy,
                                      const int32_t *arg, int64_t ldarg, float *dS, int64_t ldds, const int32_t *long_rows, int32_t n_long,
                                      int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "pool_max_bwd";
    PoolArgs a{};
    if (lddy < d || ldds < d || ldarg < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (n > 0 && !row_ptr) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (int rc = set_common(a, what, n, d, row_ptr, col, long_rows, n_long, long_threshold, workspace, workspace_bytes, 1)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!dY || !dS || !arg) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    a.src = dY; a.ldsrc = lddy; a.argin = arg; a.ldargin = ldarg; a.out = dS; a.ldout = ldds;
    return dispatch<MODE_PULL>(a, float4_rows(d, {{dY, lddy}, {dS, ldds}, {arg, ldarg}}), stream);
}

extern "C" int32_t ctgcn_bn_stats_rows(void) { return BN_ROWS; }

extern "C" size_t ctgcn_bn_stats_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 0 || d < 1) return 0;
    return (size_t)((n + BN_ROWS - 1) / BN_ROWS) * (size_t)d * 2 * sizeof(double);
}

extern "C" int ctgcn_bn_stats_f32(int64_t n, int32_t d, const float *x, int64_t ldx, double eps, float *mean, float *var, float *rstd,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    const char *what = "bn_stats";
    if (n < 1 || n > INT32_MAX || d < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "need 1 <= n < 2^31 and d >= 1");
    if (!(eps >= 0.0)) return ctgcn_fail(CTGCN_E_INVALID, what, "eps must be >= 0");
    if (!x || !mean || !var || !rstd) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (ldx < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < ctgcn_bn_stats_workspace_bytes(n, d))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 8-byte aligned and hold ctgcn_bn_stats_workspace_bytes() bytes");
    const int64_t blocks = (n + BN_ROWS - 1) / BN_ROWS;
    if (blocks > 65535) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "more than 65535 * 128 rows");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)((d + BN_COLS - 1) / BN_COLS), (unsigned)blocks), dim3(BN_COLS * 4), 0, st, n, d, x, ldx,
                       (double *)workspace);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL(bn_merge_kernel, dim3((unsigned)((d + DB_COLS - 1) / DB_COLS)), dim3(DB_COLS * DB_SEGS), 0, st, n, blocks, d,
                       (const double *)workspace, eps, mean, var, rstd);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_bn_apply_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *mean, const float *rstd, const float *weight,
                                  const float *bias, int32_t relu, double p, uint64_t key, float *y, int64_t ldy, void *stream)
{
    const char *what = "bn_apply";
    if (int rc = check_bn(what, n, d, x, ldx, mean, rstd, weight, bias, relu, p)) return rc;
    if (n == 0) return CTGCN_OK;
    if (!y) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (ldy < d) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    BnArgs a{};
    set_bn(a, n, d, x, ldx, mean, rstd, weight, bias, relu, p, key);
    a.y = y; a.ldy = ldy;
    const bool v4 = float4_rows(d, {{x, ldx}, {y, ldy}, {mean, 0}, {rstd, 0}, {weight, 0}, {bias, 0}});
    a.chunks = v4 ? d / 4 : d;
    const int64_t blocks = (n * a.chunks + 255) / 256;
    if (blocks > INT32_MAX) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "more than 2^39 elements");
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(bn_apply_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bn_apply_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_bn_bwd_workspace_bytes(int64_t n, int32_t d) { return 2 * ctgcn_pool_prep_workspace_bytes(n, d); }

extern "C" int ctgcn_bn_bwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *dy, int64_t lddy, const float *mean,
                                const float *rstd, const float *weight, const float *bias, int32_t relu, double p, uint64_t key,
                                int32_t batch_stats, float *dx, int64_t lddx, float *dw, float *db, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    const char *what = "bn_bwd";
    if (int rc = check_bn(what, n, d, x, ldx, mean, rstd, weight, bias, relu, p)) return rc;
    if (batch_stats != 0 && batch_stats != 1) return ctgcn_fail(CTGCN_E_INVALID, what, "batch_stats must be 0 or 1");
    if (n == 0) return CTGCN_OK;
    if (!dy || !dw || !db) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (lddy < d || (dx && lddx < d)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension below d");
    if (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < ctgcn_bn_bwd_workspace_bytes(n, d))
        return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace must be 16-byte aligned and hold ctgcn_bn_bwd_workspace_bytes() bytes");
    BnArgs a{};
    set_bn(a, n, d, x, ldx, mean, rstd, weight, bias, relu, p, key);
    a.dy = dy; a.lddy = lddy; a.dx = dx; a.lddx = lddx; a.dw = dw; a.db = db; a.inv_n = batch_stats ? 1.0f / (float)n : 0.f;
    a.part = (float *)workspace; a.part_ld = (d + 3) & ~3; a.blocks = prep_blocks(n);
    const bool v4 = float4_rows(d, {{x, ldx}, {dy, lddy}, {dx, lddx}, {mean, 0}, {rstd, 0}, {weight, 0}, {bias, 0}, {dw, 0}, {db, 0}});
    a.chunks = v4 ? d / 4 : d;
    if ((n * a.chunks + 255) / 256 > INT32_MAX) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "more than 2^39 elements");
    hipStream_t st = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(bn_bwd_reduce_kernel<4>, dim3((unsigned)a.blocks), dim3(64 * PREP_WAVES), 0, st, a);
    else hipLaunchKernelGGL(bn_bwd_reduce_kernel<1>, dim3((unsigned)a.blocks), dim3(64 * PREP_WAVES), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    const dim3 cgrid((unsigned)((d + DB_COLS - 1) / DB_COLS));
    hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), cgrid, dim3(DB_COLS * DB_SEGS), 0, st, a.blocks, d, a.part_ld, (const float *)a.part, db);
    CTGCN_TRY(hipGetLastError());
    hipLaunchKernelGGL((colsum_kernel<DB_COLS, DB_SEGS>), cgrid, dim3(DB_COLS * DB_SEGS), 0, st, a.blocks, d, a.part_ld,
                       (const float *)a.part + a.blocks * a.part_ld, dw);
    CTGCN_TRY(hipGetLastError());
    if (!dx) return CTGCN_OK;
    const int64_t blocks = (n * a.chunks + 255) / 256;
    if (v4) hipLaunchKernelGGL(bn_bwd_dx_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bn_bwd_dx_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
