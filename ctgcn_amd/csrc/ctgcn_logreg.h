// ctgcn_logreg.h — device helpers of the logistic-regression kernels (ctgcn_eval.hip, ctgcn_nodecls.hip; ctgcn_epoch.hip takes the two
// scalar functions): fp64 sigmoid / softplus, and the pieces of the Hessian kernels that do not depend on how a tile is staged.
//
// A Hessian block of 256 threads accumulates Σ a_e f_e f_eᵀ over tiles of 32 rows f_e = (features, 1, 0...) of width D4 = (d+1) rounded
// up to 4.  The upper triangle of the nb x nb grid of 4 x 4 blocks (nb = D4 / 4) is dealt to the threads in row-major order, MAXB blocks
// per thread; each keeps its blocks in registers across the tiles.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ double sigmoid(double x)
{
    if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
    const double e = exp(x);
    return e / (1.0 + e);
}
__device__ __forceinline__ double softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// The L-th block of the upper triangle in row-major order: (j, k) with j <= k; (-1, -1) past the last.
__device__ __forceinline__ void hess_block(int L, int nb, int ntri, int &j, int &k)
{
    int r = 0;
    if (L >= ntri) { j = k = -1; return; }
    while (L >= nb - r) { L -= nb - r; ++r; }
    j = r;
    k = r + L;
}

// Thread t's blocks are number t + q·THREADS, q < MAXB.  acc is zeroed.
template <int MAXB, int THREADS>
__device__ __forceinline__ void hess_blocks(int nb, int ntri, int (&bj)[MAXB], int (&bk)[MAXB], float (&acc)[MAXB][16])
{
#pragma unroll
    for (int q = 0; q < MAXB; ++q) hess_block(threadIdx.x + q * THREADS, nb, ntri, bj[q], bk[q]);
#pragma unroll
    for (int q = 0; q < MAXB; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
}

// z = f·w of tile row threadIdx.x / 8 (F [rows, D4] in LDS, w [D1]): 8 lanes per row, fixed-order butterfly; every lane gets the sum.
__device__ __forceinline__ float hess_row_z(const float *F, int D4, int D1, const float *__restrict__ w)
{
    const int ee = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float zp = 0.f;
    for (int c = sub; c < D1; c += 8) zp += F[ee * D4 + c] * w[c];
    zp += __shfl_xor(zp, 1, 64);
    zp += __shfl_xor(zp, 2, 64);
    zp += __shfl_xor(zp, 4, 64);
    return zp;
}

// a = s σ(z)(1 - σ(z)): the curvature of a row of weight s
__device__ __forceinline__ float hess_curvature(double s, float z)
{
    const double sg = sigmoid((double)z);
    return (float)(s * sg * (1.0 - sg));
}

// acc += Aw[e] · f_e f_eᵀ on the thread's blocks, over the TE rows of the staged tile
template <int MAXB, int TE>
__device__ __forceinline__ void hess_accumulate(const float *F, int D4, const float *Aw, const int (&bj)[MAXB], const int (&bk)[MAXB],
                                                float (&acc)[MAXB][16])
{
    for (int ee = 0; ee < TE; ++ee) {
        const float a = Aw[ee];
        const float *fr = F + ee * D4;
#pragma unroll
        for (int q = 0; q < MAXB; ++q) {
            if (bj[q] < 0) continue;
            const float4 fj = *reinterpret_cast<const float4 *>(fr + 4 * bj[q]);
            const float4 fk = *reinterpret_cast<const float4 *>(fr + 4 * bk[q]);
            const float tj[4] = {a * fj.x, a * fj.y, a * fj.z, a * fj.w}, tk[4] = {fk.x, fk.y, fk.z, fk.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[q][r * 4 + c] += tj[r] * tk[c];
        }
    }
}

// out[j·D1 + k] = the thread's entries with j <= k < D1 (out: one model's [D1, D1] partial)
template <int MAXB>
__device__ __forceinline__ void hess_store_upper(float *out, int D1, const int (&bj)[MAXB], const int (&bk)[MAXB],
                                                 const float (&acc)[MAXB][16])
{
#pragma unroll
    for (int q = 0; q < MAXB; ++q) {
        if (bj[q] < 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int jj = 4 * bj[q] + r, kk = 4 * bk[q] + c;
                if (jj < D1 && kk < D1) out[jj * D1 + kk] = acc[q][r * 4 + c];
            }
    }
}
