// ctgcn_lstmcell.hip — one time step of an LSTM layer of any width, forward and backward, for the DynRNN and DynAERNN baselines
// (reference baseline/dynRNN.py, baseline/dynAERNN.py).  The products with W_ih and W_hh are the caller's GEMMs; everything between
// them is one element-wise pass here.  Gate order is torch's: i, f, g, o, so row b of a [B, 4H] operand holds four blocks of H.
//
//   forward    z = gi + gh + bias;  i, f, o = σ(z), g = tanh(z);  c = f c_prev + i g;  h = o tanh(c).  Writes h, c and, for training,
//              the four activated gates.
//   backward   dh = dh_out + dh_rec;  dc = dh o (1 − tanh²c) + dc_next;  the pre-activation gate gradients
//              (dc g i(1 − i), dc c_prev f(1 − f), dc i (1 − g²), dh tanh(c) o(1 − o)) and dc_prev = dc f.  tanh(c) is recomputed.
//
// A thread owns one float4 (or one float) of a row's H columns and with it the same columns of the four gate blocks: every element of
// every operand is read once and written once, so an output may take the memory of the input it replaces.  No LDS, no atomics; two
// calls give the same bits.  σ(z) = 1 / (1 + e^−z) and tanhf saturate to 0, 1 and ±1 without passing through inf / inf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctgcn_gather.h"
#include "ctgcn_try.h"

namespace {

constexpr int CELL_THREADS = 256;
constexpr int64_t CELL_MAX_BLOCKS = 1 << 20;    // beyond that a thread takes several items

__device__ __forceinline__ float sigmoid_of(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ f4 sigmoid_of(f4 z) { return f4{sigmoid_of(z.x), sigmoid_of(z.y), sigmoid_of(z.z), sigmoid_of(z.w)}; }
__device__ __forceinline__ float tanh_of(float z) { return tanhf(z); }
__device__ __forceinline__ f4 tanh_of(f4 z) { return f4{tanhf(z.x), tanhf(z.y), tanhf(z.z), tanhf(z.w)}; }

// the row of item q; a 32-bit division wherever the item count allows it (uniform over the launch)
__device__ __forceinline__ int64_t row_of(int64_t q, int64_t items, int32_t chunks)
{
    return items <= INT32_MAX ? (int64_t)((uint32_t)q / (uint32_t)chunks) : q / chunks;
}

template <class V> __device__ __forceinline__ V load(const float *p) { return *(const V *)p; }
template <class V> __device__ __forceinline__ void store(float *p, V v) { *(V *)p = v; }

struct CellFwdArgs {
    int64_t B, items;        // items = B chunks
    int32_t H, chunks;
    const float *gi, *gh, *bias, *c_prev;
    int64_t ldgi, ldgh, ldcp;
    float *h, *c, *gates;
    int64_t ldh, ldc, ldg;
};

template <int VEC>
__global__ __launch_bounds__(CELL_THREADS) void lstm_cell_fwd_kernel(const CellFwdArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int64_t stride = (int64_t)gridDim.x * CELL_THREADS;
    for (int64_t q = (int64_t)blockIdx.x * CELL_THREADS + threadIdx.x; q < a.items; q += stride) {
        const int64_t b = row_of(q, a.items, a.chunks);
        const int64_t j = (q - b * a.chunks) * VEC;
        const int64_t H = a.H;
        V z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = load<V>(a.gi + b * a.ldgi + k * H + j);
        if (a.gh) {
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] += load<V>(a.gh + b * a.ldgh + k * H + j);
        }
        if (a.bias) {
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] += load<V>(a.bias + k * H + j);
        }
        const V i = sigmoid_of(z[0]), f = sigmoid_of(z[1]), g = tanh_of(z[2]), o = sigmoid_of(z[3]);
        V c = i * g;
        if (a.c_prev) c += f * load<V>(a.c_prev + b * a.ldcp + j);
        store<V>(a.c + b * a.ldc + j, c);
        store<V>(a.h + b * a.ldh + j, o * tanh_of(c));
        if (a.gates) {
            float *gt = a.gates + b * a.ldg + j;
            store<V>(gt, i);
            store<V>(gt + H, f);
            store<V>(gt + 2 * H, g);
            store<V>(gt + 3 * H, o);
        }
    }
}

struct CellBwdArgs {
    int64_t B, items;
    int32_t H, chunks;
    const float *gates, *c, *c_prev, *dh_out, *dh_rec, *dc_next;
    int64_t ldg, ldc, ldcp, lddo, lddr, lddn;
    float *dgates, *dc_prev;
    int64_t lddg, lddp;
};

template <int VEC>
__global__ __launch_bounds__(CELL_THREADS) void lstm_cell_bwd_kernel(const CellBwdArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int64_t stride = (int64_t)gridDim.x * CELL_THREADS;
    for (int64_t q = (int64_t)blockIdx.x * CELL_THREADS + threadIdx.x; q < a.items; q += stride) {
        const int64_t b = row_of(q, a.items, a.chunks);
        const int64_t j = (q - b * a.chunks) * VEC;
        const int64_t H = a.H;
        const float *gt = a.gates + b * a.ldg + j;
        const V i = load<V>(gt), f = load<V>(gt + H), g = load<V>(gt + 2 * H), o = load<V>(gt + 3 * H);
        const V tc = tanh_of(load<V>(a.c + b * a.ldc + j));
        V dh = V(0.f), dc = V(0.f), cp = V(0.f);
        if (a.dh_out) dh = load<V>(a.dh_out + b * a.lddo + j);
        if (a.dh_rec) dh += load<V>(a.dh_rec + b * a.lddr + j);
        if (a.dc_next) dc = load<V>(a.dc_next + b * a.lddn + j);
        if (a.c_prev) cp = load<V>(a.c_prev + b * a.ldcp + j);
        dc += dh * o * (1.f - tc * tc);
        float *dg = a.dgates + b * a.lddg + j;
        store<V>(dg, dc * g * i * (1.f - i));
        store<V>(dg + H, dc * cp * f * (1.f - f));
        store<V>(dg + 2 * H, dc * i * (1.f - g * g));
        store<V>(dg + 3 * H, dh * tc * o * (1.f - o));
        if (a.dc_prev) store<V>(a.dc_prev + b * a.lddp + j, dc * f);
    }
}

template <class Args> dim3 cell_grid(Args &a, int vec)
{
    a.chunks = (a.H + vec - 1) / vec;
    a.items = a.B * a.chunks;
    const int64_t blocks = (a.items + CELL_THREADS - 1) / CELL_THREADS;
    return dim3((unsigned)(blocks > CELL_MAX_BLOCKS ? CELL_MAX_BLOCKS : blocks));
}

}  // namespace

extern "C" int ctgcn_lstm_cell_fwd_f32(int64_t B, int32_t H, const float *gi, int64_t ldgi, const float *gh, int64_t ldgh, const float *bias,
                                       const float *c_prev, int64_t ldcp, float *h, int64_t ldh, float *c, int64_t ldc, float *gates,
                                       int64_t ldg, void *stream)
{
    const char *what = "lstm_cell_fwd";
    if (B < 0 || B > INT32_MAX || H < 1 || H > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= B < 2^31 and 1 <= H < 2^29");
    const int64_t H4 = 4 * (int64_t)H;
    if (ldgi < H4 || (gh && ldgh < H4) || (gates && ldg < H4)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a gate operand below 4 H");
    if ((c_prev && ldcp < H) || ldh < H || ldc < H) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a state operand below H");
    if (B == 0) return CTGCN_OK;
    if (!gi || !h || !c) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    CellFwdArgs a{};
    a.B = B; a.H = H; a.gi = gi; a.ldgi = ldgi; a.gh = gh; a.ldgh = ldgh; a.bias = bias; a.c_prev = c_prev; a.ldcp = ldcp;
    a.h = h; a.ldh = ldh; a.c = c; a.ldc = ldc; a.gates = gates; a.ldg = ldg;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = float4_rows(H, {{gi, ldgi}, {gh, ldgh}, {bias, 0}, {c_prev, ldcp}, {h, ldh}, {c, ldc}, {gates, ldg}});
    const dim3 grid = cell_grid(a, v4 ? 4 : 1);                           // sets a.chunks and a.items
    if (v4) hipLaunchKernelGGL(lstm_cell_fwd_kernel<4>, grid, dim3(CELL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(lstm_cell_fwd_kernel<1>, grid, dim3(CELL_THREADS), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_lstm_cell_bwd_f32(int64_t B, int32_t H, const float *gates, int64_t ldg, const float *c, int64_t ldc, const float *c_prev,
                                       int64_t ldcp, const float *dh_out, int64_t lddo, const float *dh_rec, int64_t lddr,
                                       const float *dc_next, int64_t lddn, float *dgates, int64_t lddg, float *dc_prev, int64_t lddp,
                                       void *stream)
{
    const char *what = "lstm_cell_bwd";
    if (B < 0 || B > INT32_MAX || H < 1 || H > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= B < 2^31 and 1 <= H < 2^29");
    const int64_t H4 = 4 * (int64_t)H;
    if (ldg < H4 || lddg < H4) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a gate operand below 4 H");
    if (ldc < H || (c_prev && ldcp < H) || (dh_out && lddo < H) || (dh_rec && lddr < H) || (dc_next && lddn < H) || (dc_prev && lddp < H))
        return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a state operand below H");
    if (B == 0) return CTGCN_OK;
    if (!gates || !c || !dgates) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    CellBwdArgs a{};
    a.B = B; a.H = H; a.gates = gates; a.ldg = ldg; a.c = c; a.ldc = ldc; a.c_prev = c_prev; a.ldcp = ldcp; a.dh_out = dh_out; a.lddo = lddo;
    a.dh_rec = dh_rec; a.lddr = lddr; a.dc_next = dc_next; a.lddn = lddn; a.dgates = dgates; a.lddg = lddg; a.dc_prev = dc_prev; a.lddp = lddp;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = float4_rows(H, {{gates, ldg}, {c, ldc}, {c_prev, ldcp}, {dh_out, lddo}, {dh_rec, lddr}, {dc_next, lddn}, {dgates, lddg},
                                    {dc_prev, lddp}});
    const dim3 grid = cell_grid(a, v4 ? 4 : 1);                           // sets a.chunks and a.items
    if (v4) hipLaunchKernelGGL(lstm_cell_bwd_kernel<4>, grid, dim3(CELL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(lstm_cell_bwd_kernel<1>, grid, dim3(CELL_THREADS), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
