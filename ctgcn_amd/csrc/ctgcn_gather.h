// ctgcn_gather.h — the scaffold of the pull-form row gathers (ctgcn_gcn.hip, ctgcn_gat.hip, ctgcn_pool.hip); each file keeps its own
// Args struct and its row, piece and final kernels.
//
// The contract, which ops.GcnAdj sizes its long-row list and workspace by:
//   pieces      a row of more than long_threshold entries is long.  It is cut into ceil(len / (PIECE_FACTOR long_threshold)) pieces, at
//               least 1 and at most max_pieces = min(workspace_bytes / (bytes of one piece of every long row), 4096).
//   caps        at most 65535 long rows (the piece grid's y extent); 1 <= long_threshold < 2^29.
//   workspace   16-byte aligned, at least one piece of every long row; a piece's size is the caller's (floats_per_piece).
//   float4      a call takes the float4 kernels when the width and every leading dimension are multiples of 4 and every base is
//               16-byte aligned, else the scalar ones.
//   launches    the row kernel over all rows (it skips the long ones), then, with long rows, the piece kernel on a
//               (max_pieces, n_long) grid and the final kernel on n_long blocks of one wave, in that order on one stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "ctgcn_try.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int PIECE_FACTOR = 4;        // entries of a long row's piece, in units of long_threshold (ops.GCN_PIECE_FACTOR)
constexpr int PIECE_THREADS = 256;
constexpr int PIECE_LANES = 32;        // lanes across the feature row in the piece kernel
constexpr int PIECE_GROUPS = PIECE_THREADS / PIECE_LANES;
constexpr float L2_EPS = 1e-12f;       // F.normalize's eps: the denominator is max(norm, eps)
constexpr int PREP_ROWS = 64;          // rows of a backward pre-pass block: one partial column-sum vector per block
constexpr int PREP_WAVES = 4;          // wave w takes the block's rows w, w + 4, ...; its lanes lie across the feature row
constexpr int DB_COLS = 32, DB_SEGS = 32;

template <int VEC> struct vec_of;
template <> struct vec_of<4> { using type = f4; };
template <> struct vec_of<1> { using type = float; };

__device__ __forceinline__ f4 vfma(float a, f4 x, f4 acc) { return f4{fmaf(a, x.x, acc.x), fmaf(a, x.y, acc.y), fmaf(a, x.z, acc.z), fmaf(a, x.w, acc.w)}; }
__device__ __forceinline__ float vfma(float a, float x, float acc) { return fmaf(a, x, acc); }

__host__ __device__ __forceinline__ int pieces_of(int len, int long_thresh, int max_pieces)
{
    const int64_t piece = (int64_t)PIECE_FACTOR * long_thresh;
    const int64_t np = (len + piece - 1) / piece;
    return (int)(np < 1 ? 1 : (np > max_pieces ? max_pieces : np));
}

// out[c] = sum over the blocks of part[b][c]: SEGS runs of consecutive blocks, each in block order, then the runs in run order; COLS
// columns a block.  A template (launched as <DB_COLS, DB_SEGS>), so that a file which launches none carries no copy.
template <int COLS, int SEGS>
__global__ __launch_bounds__(COLS * SEGS) void colsum_kernel(int64_t blocks, int32_t d, int32_t part_ld, const float *part, float *out)
{
    __shared__ float sm[SEGS][COLS];
    const int cx = threadIdx.x % COLS, seg = threadIdx.x / COLS;
    const int64_t c = (int64_t)blockIdx.x * COLS + cx;
    const int64_t per = (blocks + SEGS - 1) / SEGS;
    const int64_t lo = min(blocks, seg * per), hi = min(blocks, lo + per);
    float t = 0.f;
    if (c < d)
        for (int64_t b = lo; b < hi; ++b) t += part[b * part_ld + c];
    sm[seg][cx] = t;
    __syncthreads();
    if (seg == 0 && c < d) {
        for (int k = 1; k < SEGS; ++k) t += sm[k][cx];
        out[c] = t;
    }
}

// p as [.][ld] rows, or a vector with ld 0; a null p is an operand the call does not have
struct Operand {
    const void *p;
    int64_t ld;
};

// float4 rows: d (for GAT the head width, so d too) and every leading dimension a multiple of 4, every base 16-byte aligned
bool float4_rows(int32_t d, std::initializer_list<Operand> operands)
{
    if (d % 4) return false;
    for (const Operand &o : operands)
        if (o.p && (o.ld % 4 || !ctgcn_aligned16(o.p))) return false;
    return true;
}

bool bad_p(double p) { return !(p >= 0.0 && p < 1.0); }

// the long-row fields of a gather's Args (long_rows, n_long, long_thresh, max_pieces, part) after their checks; the caller has checked
// n_long against [0, n].  floats_per_piece is what one piece of one row takes of the workspace, workspace_text the caller's refusal.
template <class Args>
int set_long_rows(Args &a, const char *what, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, size_t floats_per_piece,
                  void *workspace, size_t workspace_bytes, const char *workspace_text)
{
    a.long_rows = long_rows; a.n_long = n_long; a.long_thresh = long_threshold;
    if (n_long <= 0) return CTGCN_OK;
    if (!long_rows) return ctgcn_fail(CTGCN_E_INVALID, what, "n_long > 0 without long_rows");
    if (long_threshold < 1 || long_threshold > INT32_MAX / PIECE_FACTOR) return ctgcn_fail(CTGCN_E_INVALID, what, "long_threshold outside [1, 2^29)");
    if (n_long > 65535) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "more than 65535 long rows: raise long_threshold");
    const size_t one = (size_t)n_long * floats_per_piece * sizeof(float);
    if (!workspace || !ctgcn_aligned16(workspace) || workspace_bytes < one) return ctgcn_fail(CTGCN_E_WORKSPACE, what, workspace_text);
    const size_t mp = workspace_bytes / one;
    a.max_pieces = (int32_t)(mp > 4096 ? 4096 : mp);
    a.part = (float *)workspace;
    return CTGCN_OK;
}

// the launches of one gather, a.chunks set.  row(lpr, grid) launches the caller's row kernel with decltype(lpr)::value lanes per row
// on 256-thread blocks, piece(grid) its piece kernel on PIECE_THREADS threads, last(grid) its final kernel on one wave.
template <class Args, class Row, class Piece, class Last>
int launch_rows(const Args &a, Row row, Piece piece, Last last)
{
    const int lpr = a.chunks <= 4 ? 4 : a.chunks <= 8 ? 8 : a.chunks <= 16 ? 16 : a.chunks <= 32 ? 32 : 64;
    const dim3 grid((unsigned)((a.n + 256 / lpr - 1) / (256 / lpr)));
    switch (lpr) {
    case 4: row(std::integral_constant<int, 4>{}, grid); break;
    case 8: row(std::integral_constant<int, 8>{}, grid); break;
    case 16: row(std::integral_constant<int, 16>{}, grid); break;
    case 32: row(std::integral_constant<int, 32>{}, grid); break;
    default: row(std::integral_constant<int, 64>{}, grid); break;
    }
    CTGCN_TRY(hipGetLastError());
    if (a.n_long > 0) {
        piece(dim3((unsigned)a.max_pieces, (unsigned)a.n_long));
        CTGCN_TRY(hipGetLastError());
        last(dim3((unsigned)a.n_long));
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}

}  // namespace
