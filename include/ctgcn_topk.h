/*
 * ctgcn_topk.h — C ABI of the top-k link ranking (ctgcn_topk.hip), an extension of include/ctgcn_hip.h in the same library
 * (libctgcn_hip.so) under the same conventions: device pointers, an explicit stream, caller-provided workspaces, 0 or a negative
 * CTGCN_E_* code of ctgcn_hip.h as return value, the text of the failure in ctgcn_last_error().  It has a header of its own because
 * the set of entry points that ctgcn_hip.h declares is pinned (ABI 31); ctgcn_amd/_lib.py reads both files with the same reader
 * (ctgcn_amd/_cdecl.py) and binds both.
 */
#ifndef CTGCN_TOPK_H
#define CTGCN_TOPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ops.topk_scores, evaluation/graph_reconstruction.py: for the query rows i = 0 .. m-1
 * the k best admissible candidate nodes and their scores, without the [m, n] score matrix.  Query i is node q = rows[i] (int32, in
 * [0, n); the caller checks that), or q = i with rows null (then m <= n).  Candidates are the n rows of E [n, d] (fp32, row stride lde).
 * Score: acc = +0; acc = fmaf(E[q, t], E[j, t], acc) for t = 0 .. d-1 ascending (on the exact-fp32 matrix cores, one accumulator);
 *   then s = acc + col_bias[j] (fp32, n entries, or null), then s = s + row_bias[i] (fp32, m entries, or null).  A pair's score does
 *   not depend on the tiling or on col_chunks.  A chain that ends on -0 may be returned as +0.  Inputs are finite.
 * Admissible: every j in [0, n) except j == q under CTGCN_TOPK_NO_SELF, j <= q under CTGCN_TOPK_UPPER, and the stored entries of row q
 *   of the exclusion CSR (int32 ex_row_ptr[n + 1] / ex_col indexed by node id, columns ascending within a row; both null: none).
 * Order: higher score first, the lower j among equal scores; score [m, k] and index [m, k] (dense) hold each row in that order, and
 *   where fewer than k candidates are admissible the tail holds score -inf and index -1.
 * The column tiles are cut into col_chunks pieces (grid = row tiles x col_chunks, which lets a small m fill the device); with more
 *   than one the partial lists go to the workspace (ctgcn_topk_workspace_bytes, 8-byte aligned) and a second kernel merges them in
 *   the same total order.  No float atomics: the result is bit-identical when repeated and for every col_chunks.  64-bit offsets;
 *   rows of E are read 16 bytes at a time when d and lde are multiples of 4 and E is 16-byte aligned, element by element otherwise.
 * Returns CTGCN_E_INVALID for negative sizes, d, k or col_chunks below 1, lde < d, an unknown flag, m > n without rows, one exclusion
 * pointer without the other and null pointers; CTGCN_E_UNSUPPORTED for k > ctgcn_topk_max_k() (128), d > ctgcn_topk_max_d() (512),
 * col_chunks > 256 and m or n >= 2^31; CTGCN_E_WORKSPACE for a workspace that is too small; all before any launch.  m = 0 returns
 * CTGCN_OK after the size checks.
 */
#define CTGCN_TOPK_NO_SELF 1
#define CTGCN_TOPK_UPPER 2
int32_t ctgcn_topk_max_k(void);
int32_t ctgcn_topk_max_d(void);
size_t ctgcn_topk_workspace_bytes(int64_t m, int64_t n, int32_t k, int32_t col_chunks);
int ctgcn_topk_scores_f32(int64_t m, int64_t n, int32_t d, int32_t k, const float *E, int64_t lde, const int32_t *rows,
                          const float *row_bias, const float *col_bias, const int32_t *ex_row_ptr, const int32_t *ex_col, int32_t flags,
                          int32_t col_chunks, float *score, int32_t *index, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CTGCN_TOPK_H */
