// ctgcn_pgnn.hip — the P-GNN baseline (reference baseline/pgnn.py) on the GPU: anchor distances and the message pass.
//
//   anchor dist  for A anchor sets at once, a level-synchronous multi-source BFS over the CSR pattern.  label[v, a] is the smallest
//                position (inside set a) of an anchor closest to v, level[v, a] its distance.  A pass for level L is a pull: an
//                unreached (v, a) scans v's row and takes the smallest label among neighbours whose level is L.  A pass writes only
//                L + 1 into level[] and labels of nodes it reaches, and reads labels only of nodes at level L, which the previous pass
//                finished: in place, no atomics in the passes, independent of the order of execution.  Seeding uses an integer
//                atomicMin on the label (a member listed twice keeps its smallest position; the minimum is order-independent).
//                The set index is the fast axis: neighbouring lanes share a CSR row and read one contiguous run of labels.
//                dist_max = 1 / (level + 1) in fp32 (0 unreached) and dist_argmax = label (0 unreached) are what the reference's
//                np.max / np.argmax over the [N, N] matrix of 1 / (d + 1) give, without that matrix.
//   conv fwd     per node n and anchor set a: m = relu(d'[n, a] P[idx[n, a]] + S[n]) in registers, P | S = PS the two halves of
//                F [W1 ; W2]^T (+ b in S); pos[n, a] = <m, w_p> + b_p and struct[n] = mean_a m.  Epilogues: the L2 normalisation of
//                pos rows, counter-based dropout on struct (ctgcn_rng.h).  d' = table[lvl[n, a]].
//   conv bwd     a row pass (gS, gd', the normalisation's backward, block partials of g_w_p and g_b_p), a pull pass over the
//                transposed index (for node j the (n, a) that chose it, cut into pieces) for gP, and a segmented sum of gd' over
//                the table index for g_table.  Everything per (n, a, channel) is recomputed; nothing of N x A x out is stored.
//
// A wave owns a node (or a piece of a pull list); LPR lanes lie across the channels, each with CPL of them, and the 64 / LPR lane
// groups take interleaved anchor sets (items).  Sums across lanes are xor butterflies, sums across blocks and pieces are added in
// index order by a second launch: no float atomics, repeated launches are bit-identical.
//
// The long sums are kept in fp64 (products and the values written are fp32).  They cancel heavily on real anchor draws: most (node, set)
// pairs are unreached and gather one and the same row, so a normalised position row is nearly constant, its gradient is nearly
// orthogonal to it, and sum_a gm is a small difference of large terms whose fp32 accumulation error shows in the weight gradients.
// For the same reason the normalisation's backward works in fp64 from the position output before the normalisation, which the forward
// saves: equal entries of the normalised row would all carry the same rounding error, which a sum over them does not average out.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "ctgcn_rng.h"
#include "ctgcn_try.h"

namespace {

constexpr int UNREACHED = 0x7fffffff;
constexpr float L2_EPS = 1e-12f;       // F.normalize's eps: the denominator is max(norm, eps)
constexpr int MAX_D = 512;
constexpr int BWD_ROWS_PER_WAVE = 4;   // rows a wave of the backward's row pass walks: one partial g_w_p vector per 16 rows
constexpr int MAX_GRID = 1 << 20;

// ------------------------------------------------------------------------------------------------ anchor distances
struct DistArgs {
    int64_t n, total, nnz;             // total = n * A
    int32_t A, n_members;
    const int32_t *row_ptr, *col, *offsets, *members;
    int32_t *level, *label;            // [n, A]
    float *dist;
    int32_t *node;                     // or null
    int32_t *flags;                    // [0] a pass reached something, [1] bad offsets or members
};

__global__ __launch_bounds__(256) void dist_init_kernel(const DistArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        a.level[i] = -1;
        a.label[i] = UNREACHED;
    }
}

// thread e: member e of the packed list, and the monotonicity of offsets[e], offsets[e + 1]
__global__ __launch_bounds__(256) void dist_seed_kernel(const DistArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < a.A && a.offsets[e] > a.offsets[e + 1]) a.flags[1] = 1;
    if (e == 0 && (a.offsets[0] != 0 || a.offsets[a.A] != a.n_members)) a.flags[1] = 1;
    if (e >= a.n_members) return;
    int lo = 0, hi = a.A;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int m = a.members[e];
    if (a.offsets[lo] > e || a.offsets[lo + 1] <= e || m < 0 || m >= a.n) {
        a.flags[1] = 1;
        return;
    }
    const int64_t at = (int64_t)m * a.A + lo;
    atomicMin(a.label + at, (int)(e - a.offsets[lo]));
    a.level[at] = 0;
}

__global__ __launch_bounds__(256) void dist_level_kernel(const DistArgs a, const int32_t L)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        if (a.level[i] != -1) continue;
        const int64_t v = i / a.A;
        const int s = (int)(i - v * a.A);
        int64_t lo = a.row_ptr[v], hi = a.row_ptr[v + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > a.nnz ? a.nnz : hi;
        int best = UNREACHED;
        for (int64_t e = lo; e < hi; ++e) {
            const int u = a.col[e];
            if ((uint32_t)u >= (uint64_t)a.n) continue;
            const int64_t q = (int64_t)u * a.A + s;
            if (a.level[q] == L) best = min(best, a.label[q]);
        }
        if (best != UNREACHED) {
            a.label[i] = best;
            a.level[i] = L + 1;
            a.flags[0] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void dist_final_kernel(const DistArgs a)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const int lv = a.level[i];
        const int pos = lv >= 0 ? a.label[i] : 0;
        a.label[i] = pos;
        a.dist[i] = lv >= 0 ? 1.0f / (float)(lv + 1) : 0.f;
        if (a.node) {
            const int s = (int)(i % a.A);
            const int at = a.offsets[s] + pos;
            a.node[i] = at < a.offsets[s + 1] ? a.members[at] : 0;          // an empty set has no member 0
        }
    }
}

int grid_for(int64_t items)
{
    const int64_t b = (items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > MAX_GRID ? MAX_GRID : b));
}

// ------------------------------------------------------------------------------------------------ the layer
struct ConvArgs {
    int64_t n;
    int32_t A, d, U;
    const float *PS;                   // [n, 2 d]: P | S
    int64_t ldps;
    const int32_t *lvl, *idx;          // [n, A]
    const float *table;                // [U]
    const float *w, *b;                // linear_out_position: [d], [1] or null
    // forward
    float *pos, *strct;                // [n, A], [n, d]; either may be null
    int64_t lds;
    int32_t normalize, drop;
    float *xraw;                       // [n, A]: with normalize, pos before the normalisation (the forward saves it for the backward)
    double p;
    float scale;
    uint64_t key;
    // backward
    const float *gpos;                 // d loss / d pos (after the normalisation when normalize)
    const float *gstruct;
    int64_t ldgs;
    float *gPS;                        // [n, 2 d]: the row pass writes the S half, the pull pass the P half
    int64_t ldg;
    float *gd, *gx;                    // [n, A]: d loss / d d', and d loss / d (pos before the normalisation) when normalize
    float *gse;                        // [n, d], with gstruct: struct_grad of every entry, which the pull pass reads
    int64_t ldgse;
    float *part;                       // row pass: [blocks][d + 1]; pull pass: [part rows][d]
    // pull pass
    const int32_t *perm;               // the (n, a) items n A + a sorted by idx
    const int32_t *pieces;             // [4][n_pieces]: node, lo, hi, dst (>= 0: row of gPS, else part row -1 - dst)
    int64_t n_pieces, part_rows;       // part_rows: the rows `part` holds in the pull pass
};

__device__ __forceinline__ int clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// the gradient that reaches struct[row, c] before the mean: through the dropout draw made again, over A
__device__ __forceinline__ float struct_grad(const ConvArgs &a, int64_t row, int c)
{
    if (!a.gstruct) return 0.f;
    float g = a.gstruct[row * a.ldgs + c];
    if (a.drop) g = ctgcn_u01(a.key, (uint64_t)row, (uint64_t)c) >= a.p ? g * a.scale : 0.f;
    return g / (float)a.A;
}

template <int LPR, int CPL>
__global__ __launch_bounds__(256) void pgnn_fwd_kernel(const ConvArgs a)
{
    constexpr int NSUB = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;                                        // wave-uniform
    const int lig = lane & (LPR - 1), sub = lane / LPR;
    float s[CPL], w[CPL];
    double acc[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = lig + k * LPR;
        const bool live = c < a.d;
        s[k] = live ? a.PS[row * a.ldps + a.d + c] : 0.f;
        w[k] = live ? a.w[c] : 0.f;
        acc[k] = 0.0;
    }
    const float bp = a.b ? a.b[0] : 0.f;
    double ss = 0.0;
    for (int a0 = 0; a0 < a.A; a0 += NSUB) {
        const int an = a0 + sub;
        const bool on = an < a.A;
        int64_t j = 0;
        float dv = 0.f;
        if (on) {
            j = clampi(a.idx[row * a.A + an], (int)a.n - 1);
            dv = a.table[clampi(a.lvl[row * a.A + an], a.U - 1)];
        }
        double pd = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lig + k * LPR;
            float m = 0.f;
            if (on && c < a.d) m = fmaxf(fmaf(dv, a.PS[j * a.ldps + c], s[k]), 0.f);
            acc[k] += m;
            pd += (double)m * (double)w[k];
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) pd += __shfl_xor(pd, o, LPR);
        if (on && lig == 0 && a.pos) {
            const float pp = (float)(pd + (double)bp);
            a.pos[row * a.A + an] = pp;
            if (a.normalize) a.xraw[row * a.A + an] = pp;
            ss += (double)pp * (double)pp;
        }
    }
    if (a.strct) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            double t = acc[k];
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
            const int c = lig + k * LPR;
            if (sub == 0 && c < a.d) {
                float v = (float)(t / (double)a.A);
                if (a.drop) v = ctgcn_u01(a.key, (uint64_t)row, (uint64_t)c) >= a.p ? v * a.scale : 0.f;
                a.strct[row * a.lds + c] = v;
            }
        }
    }
    if (a.pos && a.normalize) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float den = fmaxf((float)sqrt(ss), L2_EPS);
        if (lig == 0)                                              // the entries this lane stored itself
            for (int an = sub; an < a.A; an += NSUB) a.pos[row * a.A + an] = a.pos[row * a.A + an] / den;
    }
}

// d loss / d (pos[row, an] before the normalisation)
// y = x / max(|x|, eps): dx = g / den - x <g, x> / (den^2 |x|) where |x| >= eps, g / eps below; dot = <g, x>, nrm = |x|, in fp64
__device__ __forceinline__ float pos_grad(const ConvArgs &a, int64_t at, double dot, double nrm)
{
    if (!a.gpos) return 0.f;
    const float g = a.gpos[at];
    if (!a.normalize) return g;
    if (nrm < (double)L2_EPS) return (float)((double)g / (double)L2_EPS);
    return (float)(((double)g - (double)a.xraw[at] * dot / (nrm * nrm)) / nrm);
}

template <int LPR, int CPL>
__global__ __launch_bounds__(256) void pgnn_bwd_row_kernel(const ConvArgs a)
{
    constexpr int NSUB = 64 / LPR;
    __shared__ double sm[4][MAX_D + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lig = lane & (LPR - 1), sub = lane / LPR;
    float w[CPL];
    double accw[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = lig + k * LPR;
        w[k] = c < a.d ? a.w[c] : 0.f;
        accw[k] = 0.0;
    }
    double accb = 0.0;
    for (int r = 0; r < BWD_ROWS_PER_WAVE; ++r) {
        const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * BWD_ROWS_PER_WAVE + r;
        if (row >= a.n) break;                                     // wave-uniform
        double dot = 0.0, nrm = 1.0;
        if (a.gpos && a.normalize) {
            double ss = 0.0;
            for (int an = lane; an < a.A; an += 64) {
                const double x = a.xraw[row * a.A + an];
                dot += x * (double)a.gpos[row * a.A + an];
                ss += x * x;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                dot += __shfl_xor(dot, o, 64);
                ss += __shfl_xor(ss, o, 64);
            }
            nrm = sqrt(ss);
        }
        float s[CPL], gs[CPL];
        double accs[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lig + k * LPR;
            const bool live = c < a.d;
            s[k] = live ? a.PS[row * a.ldps + a.d + c] : 0.f;
            gs[k] = live ? struct_grad(a, row, c) : 0.f;
            if (live && sub == 0 && a.gse) a.gse[row * a.ldgse + c] = gs[k];
            accs[k] = 0.0;
        }
        for (int a0 = 0; a0 < a.A; a0 += NSUB) {
            const int an = a0 + sub;
            const bool on = an < a.A;
            const int64_t at = row * a.A + an;
            int64_t j = 0;
            float dv = 0.f, gp = 0.f;
            if (on) {
                j = clampi(a.idx[at], (int)a.n - 1);
                dv = a.table[clampi(a.lvl[at], a.U - 1)];
                gp = pos_grad(a, at, dot, nrm);
            }
            double gdv = 0.0;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int c = lig + k * LPR;
                if (on && c < a.d) {
                    const float pj = a.PS[j * a.ldps + c];
                    const float m = fmaxf(fmaf(dv, pj, s[k]), 0.f);
                    const float gm = m > 0.f ? fmaf(gp, w[k], gs[k]) : 0.f;
                    accs[k] += gm;
                    gdv += (double)gm * (double)pj;
                    accw[k] += (double)m * (double)gp;
                }
            }
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) gdv += __shfl_xor(gdv, o, LPR);
            if (on && lig == 0) {
                a.gd[at] = (float)gdv;
                if (a.gx) a.gx[at] = gp;
                accb += gp;
            }
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            double v = accs[k];
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            const int c = lig + k * LPR;
            if (sub == 0 && c < a.d) a.gPS[row * a.ldg + a.d + c] = (float)v;
        }
    }
    // the block's partial g_w_p [d] and g_b_p: lane groups by butterfly, the four waves in wave order
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        double v = accw[k];
#pragma unroll
        for (int o = LPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        const int c = lig + k * LPR;
        if (sub == 0 && c < a.d) sm[wave][c] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accb += __shfl_xor(accb, o, 64);
    if (lane == 0) sm[wave][a.d] = accb;
    __syncthreads();
    for (int c = threadIdx.x; c <= a.d; c += 256)
        a.part[(int64_t)blockIdx.x * (a.d + 1) + c] = (float)(((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c]);
}

// out[c] = sum over the rows of part [rows][ld] of column c: 256 threads take contiguous runs of rows in order, then a fixed tree
__global__ __launch_bounds__(256) void column_sum_kernel(const float *part, int64_t rows, int32_t ld, float *out)
{
    __shared__ double sm[256];
    const int c = blockIdx.x;
    const int64_t per = (rows + 255) / 256;
    const int64_t lo = threadIdx.x * per, hi = lo + per < rows ? lo + per : rows;
    double v = 0.0;
    for (int64_t r = lo; r < hi; ++r) v += part[r * ld + c];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = (float)sm[0];
}

// wave per piece of a pull list: gP[j] += sum over the piece's (n, a) of d' gm(n, a)
template <int LPR, int CPL>
__global__ __launch_bounds__(256) void pgnn_bwd_pull_kernel(const ConvArgs a)
{
    constexpr int NSUB = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int64_t pc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pc >= a.n_pieces) return;                                  // wave-uniform
    const int lig = lane & (LPR - 1), sub = lane / LPR;
    const int64_t items = a.n * a.A;
    const int64_t j = clampi(a.pieces[pc], (int)a.n - 1);
    int64_t lo = a.pieces[a.n_pieces + pc], hi = a.pieces[2 * a.n_pieces + pc];
    lo = lo < 0 ? 0 : lo;
    hi = hi > items ? items : hi;
    const int dst = a.pieces[3 * a.n_pieces + pc];
    float pj[CPL], w[CPL];
    double acc[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = lig + k * LPR;
        const bool live = c < a.d;
        pj[k] = live ? a.PS[j * a.ldps + c] : 0.f;
        w[k] = live ? a.w[c] : 0.f;
        acc[k] = 0.0;
    }
    for (int64_t i = lo + sub; i < hi; i += NSUB) {
        const int64_t q = clampi(a.perm[i], (int)(items - 1));
        const int64_t row = q / a.A;
        const float dv = a.table[clampi(a.lvl[q], a.U - 1)];
        const float gp = a.gx ? a.gx[q] : 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lig + k * LPR;
            if (c < a.d) {
                const float m = fmaf(dv, pj[k], a.PS[row * a.ldps + a.d + c]);
                const float gm = m > 0.f ? fmaf(gp, w[k], a.gse ? a.gse[row * a.ldgse + c] : 0.f) : 0.f;
                acc[k] += (double)dv * (double)gm;
            }
        }
    }
    if (dst < 0 && -1 - (int64_t)dst >= a.part_rows) return;      // a workspace row that does not exist (wave-uniform): nothing is written
    float *out = dst >= 0 ? a.gPS + (int64_t)clampi(dst, (int)a.n - 1) * a.ldg : a.part + (int64_t)(-1 - dst) * a.d;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = LPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        const int c = lig + k * LPR;
        if (sub == 0 && c < a.d) out[c] = (float)v;
    }
}

// block per node whose list has several pieces: its part rows ptr[i] .. ptr[i + 1] in order
__global__ __launch_bounds__(256) void pgnn_pull_final_kernel(const float *part, int32_t d, const int32_t *node, const int32_t *ptr, int64_t n,
                                                              int64_t part_rows, float *gPS, int64_t ldg)
{
    const int j = node[blockIdx.x];
    if (j < 0 || j >= n) return;
    int64_t lo = ptr[blockIdx.x], hi = ptr[blockIdx.x + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > part_rows ? part_rows : hi;
    for (int c = threadIdx.x; c < d; c += 256) {
        double v = 0.0;
        for (int64_t r = lo; r < hi; ++r) v += part[r * d + c];
        gPS[(int64_t)j * ldg + c] = (float)v;
    }
}

// block per piece of a table entry's item list: part[piece] = sum of gd over the piece, strided by thread, then a fixed tree
__global__ __launch_bounds__(256) void table_piece_kernel(const float *gd, const int32_t *perm, const int32_t *pieces, int64_t n_pieces,
                                                          int64_t items, float *part)
{
    __shared__ double sm[256];
    const int64_t pc = blockIdx.x;
    int64_t lo = pieces[pc], hi = pieces[n_pieces + pc];
    lo = lo < 0 ? 0 : lo;
    hi = hi > items ? items : hi;
    double v = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) v += gd[clampi(perm[i], (int)(items - 1))];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[pc] = (float)sm[0];
}

__global__ __launch_bounds__(256) void table_final_kernel(const float *part, const int32_t *ptr, int32_t U, int64_t n_pieces, float *g_table)
{
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    int64_t lo = ptr[u], hi = ptr[u + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_pieces ? n_pieces : hi;
    double v = 0.0;
    for (int64_t r = lo; r < hi; ++r) v += part[r];
    g_table[u] = (float)v;
}

enum { K_FWD, K_ROW, K_PULL };

template <int LPR, int CPL>
hipError_t launch_one(int kind, const ConvArgs &a, int64_t blocks, hipStream_t st)
{
    if (kind == K_FWD) pgnn_fwd_kernel<LPR, CPL><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    else if (kind == K_ROW) pgnn_bwd_row_kernel<LPR, CPL><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    else pgnn_bwd_pull_kernel<LPR, CPL><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(a);
    return hipGetLastError();
}

// the narrowest lane group that covers d with one channel per lane, then more channels per lane
hipError_t launch_conv(int kind, const ConvArgs &a, int64_t blocks, hipStream_t st)
{
    if (a.d <= 8) return launch_one<8, 1>(kind, a, blocks, st);
    if (a.d <= 16) return launch_one<16, 1>(kind, a, blocks, st);
    if (a.d <= 32) return launch_one<32, 1>(kind, a, blocks, st);
    if (a.d <= 64) return launch_one<64, 1>(kind, a, blocks, st);
    if (a.d <= 128) return launch_one<64, 2>(kind, a, blocks, st);
    if (a.d <= 256) return launch_one<64, 4>(kind, a, blocks, st);
    return launch_one<64, 8>(kind, a, blocks, st);
}

int64_t row_blocks(int64_t n) { return (n + 4 * BWD_ROWS_PER_WAVE - 1) / (4 * BWD_ROWS_PER_WAVE); }

// the checks every layer entry shares; 1: nothing to do
int check_conv(int64_t n, int32_t A, int32_t d, int32_t U, const void *PS, int64_t ldps, const void *lvl, const void *table, const void *idx,
               const void *w, double p, const char *what)
{
    char buf[160];
    if (n < 0 || n >= (int64_t)1 << 31 || A < 1 || d < 1 || U < 1 || ldps < 2 * (int64_t)d || !(p >= 0.0 && p < 1.0)) {
        snprintf(buf, sizeof(buf), "%s: bad sizes (n, A >= 1, d >= 1, U >= 1, ldps >= 2 d, p in [0, 1))", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    if (d > MAX_D) {
        snprintf(buf, sizeof(buf), "%s: d above %d", what, MAX_D);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (n == 0) return 1;
    if (n * A >= (int64_t)1 << 31) {
        snprintf(buf, sizeof(buf), "%s: n A reaches 2^31", what);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (!PS || !lvl || !table || !idx || !w) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return ctgcn_set_error_(CTGCN_E_INVALID, buf);
    }
    return CTGCN_OK;
}

} // namespace

extern "C" size_t ctgcn_pgnn_dist_workspace_bytes(void) { return 16; }

extern "C" int ctgcn_pgnn_anchor_dist(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, int32_t n_sets,
                                      const int32_t *offsets, const int32_t *members, int32_t n_members, int32_t cutoff, int32_t *level,
                                      float *dist_max, int32_t *pos, int32_t *node_id, int32_t *levels_run_host, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (n < 0 || n >= (int64_t)1 << 31 || nnz < 0 || nnz >= (int64_t)1 << 31 || n_sets < 1 || n_members < 0)
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_anchor_dist: bad sizes (0 <= n, nnz < 2^31, n_sets >= 1, n_members >= 0)");
    if (levels_run_host) *levels_run_host = 0;
    if (n == 0) return CTGCN_OK;
    if (n * n_sets >= (int64_t)1 << 31) return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, "ctgcn_pgnn_anchor_dist: n n_sets reaches 2^31");
    if (!row_ptr || (!col && nnz > 0) || !offsets || (!members && n_members > 0) || !level || !dist_max || !pos)
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_anchor_dist: null pointer");
    if (!workspace || workspace_bytes < ctgcn_pgnn_dist_workspace_bytes())
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ctgcn_pgnn_anchor_dist: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    DistArgs a;
    a.n = n;
    a.total = n * n_sets;
    a.nnz = nnz;
    a.A = n_sets;
    a.n_members = n_members;
    a.row_ptr = row_ptr;
    a.col = col;
    a.offsets = offsets;
    a.members = members;
    a.level = level;
    a.label = pos;
    a.dist = dist_max;
    a.node = node_id;
    a.flags = (int32_t *)workspace;
    const int grid = grid_for(a.total);
    int32_t host[2] = {0, 0};
    CTGCN_TRY(hipMemsetAsync(a.flags, 0, 8, st));
    dist_init_kernel<<<dim3(grid), dim3(256), 0, st>>>(a);
    CTGCN_TRY(hipGetLastError());
    const int64_t seeds = n_members > n_sets + 1 ? n_members : n_sets + 1;
    dist_seed_kernel<<<dim3(grid_for(seeds)), dim3(256), 0, st>>>(a);
    CTGCN_TRY(hipGetLastError());
    CTGCN_TRY(hipMemcpyAsync(host, a.flags, 8, hipMemcpyDeviceToHost, st));
    CTGCN_TRY(hipStreamSynchronize(st));
    if (host[1]) return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_anchor_dist: offsets not ascending from 0 to n_members, or a member outside [0, n)");
    int32_t L = 0;
    for (; cutoff <= 0 || L < cutoff; ++L) {                       // a pass reaches level L + 1; the last one finds nothing
        CTGCN_TRY(hipMemsetAsync(a.flags, 0, 4, st));
        dist_level_kernel<<<dim3(grid), dim3(256), 0, st>>>(a, L);
        CTGCN_TRY(hipGetLastError());
        CTGCN_TRY(hipMemcpyAsync(host, a.flags, 4, hipMemcpyDeviceToHost, st));
        CTGCN_TRY(hipStreamSynchronize(st));
        if (!host[0]) break;
    }
    if (levels_run_host) *levels_run_host = L;
    dist_final_kernel<<<dim3(grid), dim3(256), 0, st>>>(a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_pgnn_conv_fwd_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl,
                                       const float *table, int32_t n_table, const int32_t *idx, const float *w_p, const float *b_p, float *pos,
                                       float *strct, int64_t ldstruct, int32_t normalize, float *xraw, double p, uint64_t key, void *stream)
{
    const int rc = check_conv(n, n_sets, d, n_table, PS, ldps, lvl, table, idx, w_p, p, "ctgcn_pgnn_conv_fwd_f32");
    if (rc) return rc < 0 ? rc : CTGCN_OK;
    if ((!pos && !strct) || (strct && ldstruct < d) || (pos && normalize && !xraw))
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_conv_fwd_f32: no output asked for, ldstruct below d, or normalize without xraw");
    ConvArgs a = {};
    a.n = n;
    a.A = n_sets;
    a.d = d;
    a.U = n_table;
    a.PS = PS;
    a.ldps = ldps;
    a.lvl = lvl;
    a.idx = idx;
    a.table = table;
    a.w = w_p;
    a.b = b_p;
    a.pos = pos;
    a.strct = strct;
    a.lds = ldstruct;
    a.normalize = normalize ? 1 : 0;
    a.drop = p > 0.0 ? 1 : 0;
    a.xraw = xraw;
    a.p = p;
    a.scale = (float)(1.0 / (1.0 - p));
    a.key = key;
    CTGCN_TRY(launch_conv(K_FWD, a, (n + 3) / 4, (hipStream_t)stream));
    return CTGCN_OK;
}

extern "C" size_t ctgcn_pgnn_bwd_row_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 1 || d < 1) return 0;
    return (size_t)row_blocks(n) * (size_t)(d + 1) * sizeof(float);
}

extern "C" int ctgcn_pgnn_conv_bwd_row_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl,
                                           const float *table, int32_t n_table, const int32_t *idx, const float *w_p, const float *g_pos,
                                           const float *xraw, int32_t normalize, const float *g_struct, int64_t ldgs, double p,
                                           uint64_t key, float *gPS, int64_t ldg, float *gd, float *gx, float *gse, int64_t ldgse, float *g_w, float *g_b,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_conv(n, n_sets, d, n_table, PS, ldps, lvl, table, idx, w_p, p, "ctgcn_pgnn_conv_bwd_row_f32");
    if (rc < 0) return rc;
    if (!g_w || !g_b) return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_conv_bwd_row_f32: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (rc) {
        CTGCN_TRY(hipMemsetAsync(g_w, 0, sizeof(float) * d, st));
        CTGCN_TRY(hipMemsetAsync(g_b, 0, sizeof(float), st));
        return CTGCN_OK;
    }
    if (!gPS || !gd || ldg < 2 * (int64_t)d || (g_struct && (ldgs < d || !gse || ldgse < d)) ||
        (g_pos && normalize && (!xraw || !gx)))
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_conv_bwd_row_f32: null pointer or a leading dimension too small");
    if (!workspace || workspace_bytes < ctgcn_pgnn_bwd_row_workspace_bytes(n, d))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ctgcn_pgnn_conv_bwd_row_f32: workspace too small");
    ConvArgs a = {};
    a.n = n;
    a.A = n_sets;
    a.d = d;
    a.U = n_table;
    a.PS = PS;
    a.ldps = ldps;
    a.lvl = lvl;
    a.idx = idx;
    a.table = table;
    a.w = w_p;
    a.normalize = (normalize && g_pos) ? 1 : 0;
    a.drop = p > 0.0 ? 1 : 0;
    a.xraw = (float *)xraw;
    a.p = p;
    a.scale = (float)(1.0 / (1.0 - p));
    a.key = key;
    a.gpos = g_pos;
    a.gstruct = g_struct;
    a.ldgs = ldgs;
    a.gPS = gPS;
    a.ldg = ldg;
    a.gd = gd;
    a.gx = a.normalize ? gx : nullptr;
    a.gse = g_struct ? gse : nullptr;
    a.ldgse = ldgse;
    a.part = (float *)workspace;
    const int64_t blocks = row_blocks(n);
    CTGCN_TRY(launch_conv(K_ROW, a, blocks, st));
    column_sum_kernel<<<dim3(d), dim3(256), 0, st>>>(a.part, blocks, d + 1, g_w);
    CTGCN_TRY(hipGetLastError());
    column_sum_kernel<<<dim3(1), dim3(256), 0, st>>>(a.part + d, blocks, d + 1, g_b);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" size_t ctgcn_pgnn_bwd_pull_workspace_bytes(int64_t part_rows, int32_t d)
{
    if (part_rows < 1 || d < 1) return 0;
    return (size_t)part_rows * (size_t)d * sizeof(float);
}

extern "C" int ctgcn_pgnn_conv_bwd_pull_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl,
                                            const float *table, int32_t n_table, const float *w_p, const float *gx, const float *gse,
                                            int64_t ldgse, const int32_t *perm, const int32_t *pieces, int64_t n_pieces,
                                            const int32_t *multi_node, const int32_t *multi_ptr, int64_t n_multi, int64_t part_rows, float *gPS,
                                            int64_t ldg, void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_conv(n, n_sets, d, n_table, PS, ldps, lvl, table, perm, w_p, 0.0, "ctgcn_pgnn_conv_bwd_pull_f32");
    if (rc) return rc < 0 ? rc : CTGCN_OK;
    if (n_pieces < 0 || n_multi < 0 || part_rows < 0 || n_pieces >= (int64_t)1 << 31 || n_multi > 0x7fffffff / 2 || !gPS || ldg < 2 * (int64_t)d ||
        (gse && ldgse < d) || (n_pieces > 0 && !pieces) || (n_multi > 0 && (!multi_node || !multi_ptr)))
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_conv_bwd_pull_f32: bad piece counts, null pointer or a leading dimension too small");
    if (part_rows > 0 && (!workspace || workspace_bytes < ctgcn_pgnn_bwd_pull_workspace_bytes(part_rows, d)))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ctgcn_pgnn_conv_bwd_pull_f32: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ConvArgs a = {};
    a.n = n;
    a.A = n_sets;
    a.d = d;
    a.U = n_table;
    a.PS = PS;
    a.ldps = ldps;
    a.lvl = lvl;
    a.table = table;
    a.w = w_p;
    a.gx = (float *)gx;
    a.gse = (float *)gse;
    a.ldgse = ldgse;
    a.gPS = gPS;
    a.ldg = ldg;
    a.part = (float *)workspace;
    a.perm = perm;
    a.pieces = pieces;
    a.n_pieces = n_pieces;
    a.part_rows = part_rows;
    if (n_pieces > 0) CTGCN_TRY(launch_conv(K_PULL, a, (n_pieces + 3) / 4, st));
    if (n_multi > 0) {
        pgnn_pull_final_kernel<<<dim3((unsigned)n_multi), dim3(256), 0, st>>>(a.part, d, multi_node, multi_ptr, n, part_rows, gPS, ldg);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

extern "C" size_t ctgcn_pgnn_table_grad_workspace_bytes(int64_t n_pieces) { return n_pieces < 1 ? 0 : (size_t)n_pieces * sizeof(float); }

extern "C" int ctgcn_pgnn_table_grad_f32(int64_t items, int32_t n_table, const float *gd, const int32_t *perm, const int32_t *pieces,
                                         int64_t n_pieces, const int32_t *piece_ptr, float *g_table, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    if (items < 0 || items >= (int64_t)1 << 31 || n_table < 1 || n_pieces < 0 || n_pieces >= (int64_t)1 << 31)
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_table_grad_f32: bad sizes");
    if (!g_table || !piece_ptr || (n_pieces > 0 && (!pieces || !perm || !gd || items < 1)))
        return ctgcn_set_error_(CTGCN_E_INVALID, "ctgcn_pgnn_table_grad_f32: null pointer");
    if (n_pieces > 0 && (!workspace || workspace_bytes < ctgcn_pgnn_table_grad_workspace_bytes(n_pieces)))
        return ctgcn_set_error_(CTGCN_E_WORKSPACE, "ctgcn_pgnn_table_grad_f32: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (n_pieces > 0) {
        table_piece_kernel<<<dim3((unsigned)n_pieces), dim3(256), 0, st>>>(gd, perm, pieces, n_pieces, items, (float *)workspace);
        CTGCN_TRY(hipGetLastError());
    }
    table_final_kernel<<<dim3((n_table + 255) / 256), dim3(256), 0, st>>>((const float *)workspace, piece_ptr, n_table, n_pieces, g_table);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
