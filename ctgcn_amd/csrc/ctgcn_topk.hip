// ctgcn_topk.hip — the k best admissible partners of every query node by embedding score, without the [m, n] score matrix: the ranking
// pass of evaluation/graph_reconstruction.py (MAP and precision@k over all node pairs) and of serving (ops.topk_scores).
//
//   score    s(i, j) = fmaf chain of E[q] · E[j] over t = 0 .. d-1 ascending from +0, then + col_bias[j], then + row_bias[i], each one
//            fp32 operation.  The chain runs on the exact-fp32 matrix cores: v_mfma_f32_32x32x2_f32 adds its two products in k order,
//            one rounding each, so step p of ONE accumulator with k = (2p, 2p + 1) on the two lane halves is the chain as written.  d is
//            never split across accumulators: a pair's score does not depend on the tiling or the chunking.  (Steps are issued in
//            groups of four; the steps of a group beyond d multiply zeros, which adds +0: a chain that ends on -0 is returned as +0.)
//   sweep    a block is one wave and owns 32 query rows; it walks the 32-column tiles of its column chunk.  A = the candidates' rows,
//            B = the queries' rows, so the 16 accumulator registers of lane (r, h) hold query i = r against the candidates
//            j = J0 + (v & 3) + 8 (v >> 2) + 4 h: a query row lives on two lanes and its running k-th best (score, index) in their
//            registers.  A lane stages the candidates that are admissible and rank before that threshold in its own 32 LDS slots; a
//            tile adds at most 16, so a row whose lane holds more than 16 is merged before the next tile.
//   merge    the row's sorted list (LDS, k entries) and the two lanes' staged entries are ranked against each other by the whole wave:
//            (score descending, index ascending) is a strict total order because an index occurs once in a row, so the ranks are a
//            permutation and every entry with rank < k is stored at its rank.  No atomics, no sort network, no dependence on arrival.
//   chunks   grid = row tiles x col_chunks; chunk c owns the column tiles [T c / C, T (c + 1) / C).  With more than one chunk the
//            sorted partial lists go to the workspace and topk_merge_kernel ranks every partial entry by binary searches in the other
//            chunks' lists, in the same total order: the result is bit-identical for every col_chunks.
// Unused slots hold score -inf and index -1.  Offsets are 64-bit.  Rows of E are read as float4 when d and lde are multiples of 4 and
// the base is 16-byte aligned, element by element otherwise.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/ctgcn_topk.h"
#include "ctgcn_try.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TILE = 32;                // query rows of a wave, candidate columns of a tile
constexpr int MAX_K = 128;              // ctgcn_topk_max_k(): a merge ranks at most MAX_K + 2 STAGE = 192 entries, three a lane
constexpr int MAX_D = 512;              // ctgcn_topk_max_d()
constexpr int MAX_CHUNKS = 256;
constexpr int STAGE = 32;               // staged candidates a lane
constexpr int MERGE_THREADS = 256;
constexpr int32_t PAD = INT_MAX;        // index of an unused slot inside the kernels: it ranks after every node at score -inf

struct Ent {
    float s;
    int32_t j;
};

// the total order: higher score first, the lower index among equal scores
__device__ __forceinline__ bool before(float s, int32_t j, float os, int32_t oj) { return s > os || (s == os && j < oj); }

struct TopkArgs {
    int64_t m, n;
    int32_t d, k;
    const float *E;
    int64_t lde;
    const int32_t *rows;
    const float *row_bias, *col_bias;
    const int32_t *ex_row_ptr, *ex_col;
    int32_t flags, vec4, chunks;
    Ent *part;              // [m][chunks][k] when chunks > 1
    float *score;
    int32_t *index;
};

// the operands of steps 4 s .. 4 s + 3 of lane half h: E[row][8 s + 2 u + h], u = 0 .. 3; zero for row < 0 and beyond d
__device__ __forceinline__ v4f load_steps(const TopkArgs &a, int64_t row, int s, int h)
{
    v4f o = v4f(0.f);
    const int t0 = 8 * s;
    if (row < 0 || t0 >= a.d) return o;
    const float *p = a.E + row * a.lde + t0;
    if (a.vec4) {                                                      // d % 4 == 0: t0 < d means t0 + 3 < d
        const v4f lo = *(const v4f *)p;
        o.x = h ? lo.y : lo.x;
        o.y = h ? lo.w : lo.z;
        if (t0 + 4 < a.d) {
            const v4f hi = *(const v4f *)(p + 4);
            o.z = h ? hi.y : hi.x;
            o.w = h ? hi.w : hi.z;
        }
        return o;
    }
    if (t0 + h < a.d) o.x = p[h];
    if (t0 + 2 + h < a.d) o.y = p[2 + h];
    if (t0 + 4 + h < a.d) o.z = p[4 + h];
    if (t0 + 6 + h < a.d) o.w = p[6 + h];
    return o;
}

__device__ __forceinline__ v16f mfma4(v4f x, v4f y, v16f acc)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
    return acc;
}

// whether ascending col[lo .. hi) holds j
__device__ __forceinline__ bool csr_has(const int32_t *col, int32_t lo, int32_t hi, int32_t j)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t c = col[mid];
        if (c == j) return true;
        if (c < j) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// QS: float4 step groups of the query rows kept in registers (d <= 8 QS); 0: any d, the query rows are read again every tile
template <int QS>
__global__ __launch_bounds__(64) void topk_sweep_kernel(const TopkArgs a)
{
    extern __shared__ Ent lds[];
    Ent *list = lds;                                // [TILE][k], each row sorted, klen entries in use
    Ent *stage = lds + (size_t)TILE * a.k;          // [64][STAGE], a lane's own slots
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int k = a.k;
    const int64_t i = (int64_t)blockIdx.x * TILE + r;
    const bool i_ok = i < a.m;
    const int32_t q = i_ok ? (a.rows ? a.rows[i] : (int32_t)i) : -1;
    const int groups = (a.d + 7) / 8;

    int32_t ex_lo = 0, ex_hi = 0;
    if (i_ok && a.ex_row_ptr) {
        ex_lo = a.ex_row_ptr[q];
        ex_hi = a.ex_row_ptr[q + 1];
    }
    const float rb = (i_ok && a.row_bias) ? a.row_bias[i] : 0.f;
    const bool no_self = a.flags & CTGCN_TOPK_NO_SELF, upper = a.flags & CTGCN_TOPK_UPPER;

    // this chunk's column tiles; under UPPER the tiles at or below the wave's smallest query hold nothing admissible
    const int64_t tiles = (a.n + TILE - 1) / TILE;
    int64_t t0 = tiles * blockIdx.y / a.chunks;
    const int64_t t1 = tiles * (blockIdx.y + 1) / a.chunks;
    if (upper) {
        int32_t qmin = i_ok ? q : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) qmin = min(qmin, __shfl_xor(qmin, o, 64));
        const int64_t first = ((int64_t)qmin + 1) / TILE;
        if (first > t0) t0 = first;
    }

    v4f bq[QS ? QS : 1];
    if (QS) {
#pragma unroll
        for (int s = 0; s < QS; ++s) bq[s] = load_steps(a, q, s, h);
    }

    int cnt = 0, klen = 0;                          // staged entries of this lane; entries of row r's list (the same on both its lanes)
    float thr_s = -INFINITY;                        // the list's last entry once klen == k
    int32_t thr_j = PAD;

    // merges the rows of `rowmask` (wave-uniform): list[row] <- the best k of list[row] and the staged entries of lanes row, row + 32
    auto merge_rows = [&](uint32_t rowmask) {
        __syncthreads();                            // the staged entries are in LDS
        while (rowmask) {
            const int row = __ffs(rowmask) - 1;
            rowmask &= rowmask - 1;
            const int c0 = __shfl(cnt, row, 64), c1 = __shfl(cnt, row + 32, 64), kl = __shfl(klen, row, 64);
            const int L = kl + c0 + c1;
            const Ent *l0 = list + (size_t)row * k, *s0 = stage + row * STAGE, *s1 = stage + (row + 32) * STAGE;
            Ent mine[3];
            int rank[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int e = lane + 64 * u;
                rank[u] = 0;
                mine[u].s = -INFINITY;
                mine[u].j = PAD;
                if (e < L) mine[u] = e < kl ? l0[e] : (e < kl + c0 ? s0[e - kl] : s1[e - kl - c0]);
            }
            for (int f = 0; f < kl; ++f) {
                const Ent o = l0[f];
#pragma unroll
                for (int u = 0; u < 3; ++u) rank[u] += before(o.s, o.j, mine[u].s, mine[u].j);
            }
            for (int f = 0; f < c0; ++f) {
                const Ent o = s0[f];
#pragma unroll
                for (int u = 0; u < 3; ++u) rank[u] += before(o.s, o.j, mine[u].s, mine[u].j);
            }
            for (int f = 0; f < c1; ++f) {
                const Ent o = s1[f];
#pragma unroll
                for (int u = 0; u < 3; ++u) rank[u] += before(o.s, o.j, mine[u].s, mine[u].j);
            }
            __syncthreads();                        // every lane has read what it ranks
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (lane + 64 * u < L && rank[u] < k) list[(size_t)row * k + rank[u]] = mine[u];
            if (r == row) {
                klen = L < k ? L : k;
                cnt = 0;
            }
        }
        __syncthreads();
        if (klen == k) {
            const Ent t = list[(size_t)r * k + k - 1];
            thr_s = t.s;
            thr_j = t.j;
        }
    };

    for (int64_t jt = t0; jt < t1; ++jt) {
        const int64_t J0 = jt * TILE;
        const int64_t jrow = J0 + r < a.n ? J0 + r : -1;
        v16f x = v16f(0.f);
        if (QS) {
#pragma unroll
            for (int s = 0; s < QS; ++s)
                if (s < groups) x = mfma4(load_steps(a, jrow, s, h), bq[s], x);
        } else {
            for (int s = 0; s < groups; ++s) x = mfma4(load_steps(a, jrow, s, h), load_steps(a, q, s, h), x);
        }
        if (a.col_bias) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t j = J0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                x[v] += j < a.n ? a.col_bias[j] : 0.f;
            }
        }
        if (a.row_bias) {
#pragma unroll
            for (int v = 0; v < 16; ++v) x[v] += rb;
        }
        float mx = x[0];
#pragma unroll
        for (int v = 1; v < 16; ++v) mx = fmaxf(mx, x[v]);
        const bool full = klen == k;
        const bool cand = i_ok && (!full || mx >= thr_s);
        if (!__any(cand)) continue;
        if (cand) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t jl = J0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                const int32_t j = (int32_t)jl;
                bool ok = jl < a.n && !(no_self && j == q) && !(upper && j <= q) && (!full || before(x[v], j, thr_s, thr_j));
                if (ok && ex_hi > ex_lo) ok = !csr_has(a.ex_col, ex_lo, ex_hi, j);
                if (ok) {
                    Ent e;
                    e.s = x[v];
                    e.j = j;
                    stage[lane * STAGE + cnt] = e;
                    ++cnt;
                }
            }
        }
        const uint64_t need = __ballot(cnt > STAGE - 16);
        if (need) merge_rows((uint32_t)need | (uint32_t)(need >> 32));
    }
    {
        const uint64_t need = __ballot(cnt > 0);
        if (need) merge_rows((uint32_t)need | (uint32_t)(need >> 32));
        else __syncthreads();
    }

    // the lists leave in row order: lane e of the wave writes entry e, e + 64 of one row
    for (int row = 0; row < TILE; ++row) {
        const int64_t io = (int64_t)blockIdx.x * TILE + row;
        if (io >= a.m) break;
        const int kl = __shfl(klen, row, 64);
        for (int e = lane; e < k; e += 64) {
            Ent t;
            t.s = -INFINITY;
            t.j = PAD;
            if (e < kl) t = list[(size_t)row * k + e];
            if (a.chunks > 1) {
                a.part[(io * a.chunks + blockIdx.y) * k + e] = t;
            } else {
                a.score[io * k + e] = t.s;
                a.index[io * k + e] = t.j == PAD ? -1 : t.j;
            }
        }
    }
}

// One block a query row: every entry of the row's chunks * k partial entries finds its rank among all of them (its position in its own
// sorted list plus, by binary search, the entries of every other list that come before it) and is stored there when the rank is below k.
__global__ __launch_bounds__(MERGE_THREADS) void topk_merge_kernel(const TopkArgs a)
{
    __shared__ int real;
    const int64_t i = blockIdx.x;
    const int k = a.k, chunks = a.chunks;
    const Ent *p = a.part + i * chunks * k;
    if (threadIdx.x == 0) real = 0;
    __syncthreads();
    int mine = 0;
    for (int e = threadIdx.x; e < chunks * k; e += MERGE_THREADS) {
        const Ent t = p[e];
        if (t.j == PAD) continue;
        ++mine;
        const int c = e / k;
        int rank = e - c * k;
        for (int o = 0; o < chunks && rank < k; ++o) {
            if (o == c) continue;
            const Ent *l = p + (size_t)o * k;
            int lo = 0, hi = k;                     // the first entry of list o that does not come before t
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const Ent u = l[mid];
                if (before(u.s, u.j, t.s, t.j)) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            a.score[i * k + rank] = t.s;
            a.index[i * k + rank] = t.j;
        }
    }
    if (mine) atomicAdd(&real, mine);
    __syncthreads();
    for (int e = real + threadIdx.x; e < k; e += MERGE_THREADS) {
        a.score[i * k + e] = -INFINITY;
        a.index[i * k + e] = -1;
    }
}

template <int QS>
void launch_sweep(dim3 grid, size_t lds, hipStream_t st, const TopkArgs &a)
{
    hipLaunchKernelGGL((topk_sweep_kernel<QS>), grid, dim3(64), lds, st, a);
}

}   // namespace

extern "C" int32_t ctgcn_topk_max_k(void) { return MAX_K; }

extern "C" int32_t ctgcn_topk_max_d(void) { return MAX_D; }

extern "C" size_t ctgcn_topk_workspace_bytes(int64_t m, int64_t n, int32_t k, int32_t col_chunks)
{
    (void)n;
    if (m <= 0 || k <= 0 || col_chunks <= 1) return 0;
    return (size_t)m * (size_t)col_chunks * (size_t)k * sizeof(Ent);
}

extern "C" int ctgcn_topk_scores_f32(int64_t m, int64_t n, int32_t d, int32_t k, const float *E, int64_t lde, const int32_t *rows,
                                     const float *row_bias, const float *col_bias, const int32_t *ex_row_ptr, const int32_t *ex_col,
                                     int32_t flags, int32_t col_chunks, float *score, int32_t *index, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    const char *what = "topk_scores";
    if (m < 0 || n < 0 || d < 1 || k < 1 || col_chunks < 1) return ctgcn_fail(CTGCN_E_INVALID, what, "m, n >= 0 and d, k, col_chunks >= 1 expected");
    if (k > MAX_K) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "k above ctgcn_topk_max_k()");
    if (d > MAX_D) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "d above ctgcn_topk_max_d()");
    if (col_chunks > MAX_CHUNKS) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "col_chunks above 256");
    if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31)) return ctgcn_fail(CTGCN_E_UNSUPPORTED, what, "m and n must be below 2^31");
    if (flags & ~(CTGCN_TOPK_NO_SELF | CTGCN_TOPK_UPPER)) return ctgcn_fail(CTGCN_E_INVALID, what, "unknown flag");
    if (!rows && m > n) return ctgcn_fail(CTGCN_E_INVALID, what, "m > n without rows");
    if ((ex_row_ptr == nullptr) != (ex_col == nullptr)) return ctgcn_fail(CTGCN_E_INVALID, what, "ex_row_ptr and ex_col go together");
    if (m == 0) return CTGCN_OK;
    if (!score || !index || (n > 0 && !E)) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if (lde < d) return ctgcn_fail(CTGCN_E_INVALID, what, "lde < d");
    const size_t need = ctgcn_topk_workspace_bytes(m, n, k, col_chunks);
    if (need && (!workspace || workspace_bytes < need)) return ctgcn_fail(CTGCN_E_WORKSPACE, what, "workspace too small");
    if (need && (reinterpret_cast<uintptr_t>(workspace) & 7)) return ctgcn_fail(CTGCN_E_INVALID, what, "workspace not 8-byte aligned");

    TopkArgs a;
    a.m = m, a.n = n, a.d = d, a.k = k, a.E = E, a.lde = lde, a.rows = rows, a.row_bias = row_bias, a.col_bias = col_bias;
    a.ex_row_ptr = ex_row_ptr, a.ex_col = ex_col, a.flags = flags, a.vec4 = ctgcn_can_vec4(d, E, lde), a.chunks = col_chunks;
    a.part = static_cast<Ent *>(workspace), a.score = score, a.index = index;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((m + TILE - 1) / TILE), (unsigned)col_chunks);
    const size_t lds = ((size_t)TILE * k + 64 * STAGE) * sizeof(Ent);           // at most 48 KiB
    if (d <= 32) launch_sweep<4>(grid, lds, st, a);
    else if (d <= 64) launch_sweep<8>(grid, lds, st, a);
    else if (d <= 128) launch_sweep<16>(grid, lds, st, a);
    else launch_sweep<0>(grid, lds, st, a);
    CTGCN_TRY(hipGetLastError());
    if (col_chunks > 1) {
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)m), dim3(MERGE_THREADS), 0, st, a);
        CTGCN_TRY(hipGetLastError());
    }
    return CTGCN_OK;
}
