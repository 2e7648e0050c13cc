// ctgcn_grucell.hip — one time step of a GRU layer of any width, forward and backward: the counterpart of ctgcn_lstmcell.hip for the
// core-axis and the temporal RNN of CTGCN, CGCN and GCRN at hidden widths other than 128 (ops.gru_layer).  The products with W_ih and
// W_hh are the caller's GEMMs; everything between them is one element-wise pass here.  Gate order is torch's: r, z, n, so row b of a
// [B, 3H] operand holds three blocks of H.
//
//   forward    r = σ(gi_r + gh_r + b_hr), z = σ(gi_z + gh_z + b_hz), q = gh_n + b_hn, n = tanh(gi_n + r q), h = (1 − z) n + z h_prev.
//              Writes h and, for training, the activated gates (r, z, n) and q; with acc, the running sum of h over the steps.
//   backward   dh = dh_out + dh_rec;  dn = dh (1 − z), dz = dh (h_prev − n);  da_n = dn (1 − n²), da_z = dz z (1 − z),
//              da_r = da_n q r (1 − r);  d_gi = (da_r, da_z, da_n), d_gh = (da_r, da_z, da_n r), and the direct part dh z of dh_prev.
//
// A thread owns one float4 (or one float) of a row's H columns and with it the same columns of the three gate blocks: every element of
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

struct GruFwdArgs {
    int64_t B, items;        // items = B chunks
    int32_t H, chunks, acc_init;
    const float *gi, *gh, *b_hh, *h_prev;
    int64_t ldgi, ldgh, ldhp;
    float *h, *gates, *q, *acc;
    int64_t ldh, ldg, ldq, ldacc;
};

template <int VEC>
__global__ __launch_bounds__(CELL_THREADS) void gru_cell_fwd_kernel(const GruFwdArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int64_t stride = (int64_t)gridDim.x * CELL_THREADS;
    for (int64_t it = (int64_t)blockIdx.x * CELL_THREADS + threadIdx.x; it < a.items; it += stride) {
        const int64_t b = row_of(it, a.items, a.chunks);
        const int64_t j = (it - b * a.chunks) * VEC;
        const int64_t H = a.H;
        const float *gi = a.gi + b * a.ldgi + j;
        V ar = load<V>(gi), az = load<V>(gi + H);
        const V an = load<V>(gi + 2 * H);
        V q = V(0.f);
        if (a.gh) {
            const float *gh = a.gh + b * a.ldgh + j;
            ar += load<V>(gh);
            az += load<V>(gh + H);
            q = load<V>(gh + 2 * H);
        }
        if (a.b_hh) {
            ar += load<V>(a.b_hh + j);
            az += load<V>(a.b_hh + H + j);
            q += load<V>(a.b_hh + 2 * H + j);
        }
        const V r = sigmoid_of(ar), z = sigmoid_of(az);
        const V n = tanh_of(an + r * q);
        V h = (1.f - z) * n;
        if (a.h_prev) h += z * load<V>(a.h_prev + b * a.ldhp + j);
        store<V>(a.h + b * a.ldh + j, h);
        if (a.gates) {
            float *gt = a.gates + b * a.ldg + j;
            store<V>(gt, r);
            store<V>(gt + H, z);
            store<V>(gt + 2 * H, n);
            store<V>(a.q + b * a.ldq + j, q);
        }
        if (a.acc) {
            float *ac = a.acc + b * a.ldacc + j;
            store<V>(ac, a.acc_init ? h : load<V>(ac) + h);
        }
    }
}

struct GruBwdArgs {
    int64_t B, items;
    int32_t H, chunks;
    const float *gates, *q, *h_prev, *dh_out, *dh_rec;
    int64_t ldg, ldq, ldhp, lddo, lddr;
    float *dgi, *dgh, *dh_prev;
    int64_t lddgi, lddgh, lddp;
};

template <int VEC>
__global__ __launch_bounds__(CELL_THREADS) void gru_cell_bwd_kernel(const GruBwdArgs a)
{
    using V = typename vec_of<VEC>::type;
    const int64_t stride = (int64_t)gridDim.x * CELL_THREADS;
    for (int64_t it = (int64_t)blockIdx.x * CELL_THREADS + threadIdx.x; it < a.items; it += stride) {
        const int64_t b = row_of(it, a.items, a.chunks);
        const int64_t j = (it - b * a.chunks) * VEC;
        const int64_t H = a.H;
        const float *gt = a.gates + b * a.ldg + j;
        const V r = load<V>(gt), z = load<V>(gt + H), n = load<V>(gt + 2 * H);
        const V q = load<V>(a.q + b * a.ldq + j);
        V dh = V(0.f), hp = V(0.f);
        if (a.dh_out) dh = load<V>(a.dh_out + b * a.lddo + j);
        if (a.dh_rec) dh += load<V>(a.dh_rec + b * a.lddr + j);
        if (a.h_prev) hp = load<V>(a.h_prev + b * a.ldhp + j);
        const V dan = dh * (1.f - z) * (1.f - n * n);
        const V daz = dh * (hp - n) * z * (1.f - z);
        const V dar = dan * q * r * (1.f - r);
        float *dgi = a.dgi + b * a.lddgi + j;
        store<V>(dgi, dar);
        store<V>(dgi + H, daz);
        store<V>(dgi + 2 * H, dan);
        if (a.dgh) {
            float *dgh = a.dgh + b * a.lddgh + j;
            store<V>(dgh, dar);
            store<V>(dgh + H, daz);
            store<V>(dgh + 2 * H, dan * r);
        }
        if (a.dh_prev) store<V>(a.dh_prev + b * a.lddp + j, dh * z);
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

extern "C" int ctgcn_gru_cell_fwd_f32(int64_t B, int32_t H, const float *gi, int64_t ldgi, const float *gh, int64_t ldgh, const float *b_hh,
                                      const float *h_prev, int64_t ldhp, float *h, int64_t ldh, float *gates, int64_t ldg, float *q,
                                      int64_t ldq, float *acc, int64_t ldacc, int32_t acc_init, void *stream)
{
    const char *what = "gru_cell_fwd";
    if (B < 0 || B > INT32_MAX || H < 1 || H > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= B < 2^31 and 1 <= H < 2^29");
    const int64_t H3 = 3 * (int64_t)H;
    if (ldgi < H3 || (gh && ldgh < H3) || (gates && ldg < H3)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a gate operand below 3 H");
    if ((h_prev && ldhp < H) || ldh < H || (gates && ldq < H) || (acc && ldacc < H))
        return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a state operand below H");
    if (B == 0) return CTGCN_OK;
    if (!gi || !h) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    if ((gates == nullptr) != (q == nullptr)) return ctgcn_fail(CTGCN_E_INVALID, what, "gates and q are kept together or not at all");
    GruFwdArgs a{};
    a.B = B; a.H = H; a.gi = gi; a.ldgi = ldgi; a.gh = gh; a.ldgh = ldgh; a.b_hh = b_hh; a.h_prev = h_prev; a.ldhp = ldhp;
    a.h = h; a.ldh = ldh; a.gates = gates; a.ldg = ldg; a.q = q; a.ldq = ldq; a.acc = acc; a.ldacc = ldacc; a.acc_init = acc_init != 0;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = float4_rows(H, {{gi, ldgi}, {gh, ldgh}, {b_hh, 0}, {h_prev, ldhp}, {h, ldh}, {gates, ldg}, {q, ldq}, {acc, ldacc}});
    const dim3 grid = cell_grid(a, v4 ? 4 : 1);                           // sets a.chunks and a.items
    if (v4) hipLaunchKernelGGL(gru_cell_fwd_kernel<4>, grid, dim3(CELL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(gru_cell_fwd_kernel<1>, grid, dim3(CELL_THREADS), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}

extern "C" int ctgcn_gru_cell_bwd_f32(int64_t B, int32_t H, const float *gates, int64_t ldg, const float *q, int64_t ldq, const float *h_prev,
                                      int64_t ldhp, const float *dh_out, int64_t lddo, const float *dh_rec, int64_t lddr, float *dgi,
                                      int64_t lddgi, float *dgh, int64_t lddgh, float *dh_prev, int64_t lddp, void *stream)
{
    const char *what = "gru_cell_bwd";
    if (B < 0 || B > INT32_MAX || H < 1 || H > INT32_MAX / 4) return ctgcn_fail(CTGCN_E_INVALID, what, "need 0 <= B < 2^31 and 1 <= H < 2^29");
    const int64_t H3 = 3 * (int64_t)H;
    if (ldg < H3 || lddgi < H3 || (dgh && lddgh < H3)) return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a gate operand below 3 H");
    if (ldq < H || (h_prev && ldhp < H) || (dh_out && lddo < H) || (dh_rec && lddr < H) || (dh_prev && lddp < H))
        return ctgcn_fail(CTGCN_E_INVALID, what, "leading dimension of a state operand below H");
    if (B == 0) return CTGCN_OK;
    if (!gates || !q || !dgi) return ctgcn_fail(CTGCN_E_INVALID, what, "null pointer");
    GruBwdArgs a{};
    a.B = B; a.H = H; a.gates = gates; a.ldg = ldg; a.q = q; a.ldq = ldq; a.h_prev = h_prev; a.ldhp = ldhp; a.dh_out = dh_out; a.lddo = lddo;
    a.dh_rec = dh_rec; a.lddr = lddr; a.dgi = dgi; a.lddgi = lddgi; a.dgh = dgh; a.lddgh = lddgh; a.dh_prev = dh_prev; a.lddp = lddp;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = float4_rows(H, {{gates, ldg}, {q, ldq}, {h_prev, ldhp}, {dh_out, lddo}, {dh_rec, lddr}, {dgi, lddgi}, {dgh, lddgh},
                                    {dh_prev, lddp}});
    const dim3 grid = cell_grid(a, v4 ? 4 : 1);                           // sets a.chunks and a.items
    if (v4) hipLaunchKernelGGL(gru_cell_bwd_kernel<4>, grid, dim3(CELL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(gru_cell_bwd_kernel<1>, grid, dim3(CELL_THREADS), 0, st, a);
    CTGCN_TRY(hipGetLastError());
    return CTGCN_OK;
}
