/*
 * ctgcn_hip.h — C ABI of libctgcn_hip.so, the MI355X (gfx950) hot path of CTGCN.
 *
 * The reference (jhljx/CTGCN) is pure Python and has no FFI layer; its "operator API" for this
 * path is four call sites.  Each entry point below names the reference call site it replaces
 * (paths relative to the reference root).  A reference-side ctypes binding is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - every function returns 0 on success or a negative CTGCN_E_* code, never throws, never
 *     allocates device memory (callers pass workspaces sized by ctgcn_workspace_bytes);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); work is enqueued on it
 *     and the call returns without synchronising, except ctgcn_kcore_i32 which must read its
 *     termination counter back and therefore synchronises `stream` internally;
 *   - ctgcn_last_error() returns a thread-local, NUL-terminated description of the last failure;
 *   - CSR arrays: row_ptr int32[n_rows+1] (nnz < 2^31), col_idx int32[nnz], val float[nnz]; the per-entry
 *     arrays may be NULL when nnz == 0;
 *   - dense matrices are row-major fp32 with an explicit leading dimension (elements).
 */
#ifndef CTGCN_HIP_H
#define CTGCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTGCN_ABI_VERSION 31

enum {
    CTGCN_OK = 0,
    CTGCN_E_INVALID = -1,   /* bad argument (null pointer, negative size, K out of range ...) */
    CTGCN_E_HIP = -2,       /* a HIP runtime call failed; see ctgcn_last_error()              */
    CTGCN_E_WORKSPACE = -3, /* workspace too small                                            */
    CTGCN_E_UNSUPPORTED = -4,
    CTGCN_E_LIMIT = -5      /* an iteration cap was reached (ctgcn_lp_neg_sample)             */
};

/* flags of ctgcn_core_aggregate_f32 / ctgcn_core_aggregate_bwd_f32 */
enum {
    CTGCN_F_SELF_LOOP = 1,  /* slot 0 is (A + I): add X[row] once (helper.py:71-72)                     */
    CTGCN_F_RELU = 2,       /* apply ReLU to every emitted slot (layers.py:48)                          */
    CTGCN_F_NESTED = 4      /* edges tagged s belong to slots s..K-1 (nested k-cores).  Without it an   */
                            /* edge belongs to slot s only (arbitrary, non-nested adjacency list).      */
};

enum { /* `op` of ctgcn_workspace_bytes */
    CTGCN_OP_KCORE = 1,
    CTGCN_OP_INGEST = 2     /* pass the number of edge rows m as `nnz` */
};

#define CTGCN_MAX_SLOTS 255

/* arithmetic of the GRU matrix products (ctgcn_gru_seq_f32, ctgcn_gru_input_proj_f32) */
#define CTGCN_SPLIT_NONE 0
#define CTGCN_SPLIT_BF16X3 1
#define CTGCN_SPLIT_F16X2 2
#define CTGCN_ACT_NONE 0
#define CTGCN_ACT_SELU 1     /* torch.nn.functional.selu, layers.py:103-104 */

int ctgcn_abi_version(void);
const char *ctgcn_last_error(void);

/* Name of the device the library would run on and its compute-unit count (diagnostics). */
int ctgcn_device_info(char *name_host, size_t name_len, int *cu_count_host);

/*
 * out[n, d] = w[d, n]^T + bias[d]  — nn.Linear applied to one-hot node features (the sparse identity of reference
 * helper.py:161-172 fed to layers.py:95-106 MLP): X·W^T + b with X = I is a transpose of the weight.  w rows are ldw
 * floats apart, out rows ldo; bias may be NULL.
 */
int ctgcn_transpose_bias_f32(int64_t n, int32_t d, const float *w, int64_t ldw, const float *bias, float *out, int64_t ldo,
                             void *stream);

/*
 * Y = A·X  (accumulate == 0)   or   Y += A·X  (accumulate != 0).
 * Replaces one torch.sparse.mm(adj, x), layers.py:43 / layers.py:45.
 */
int ctgcn_spmm_csr_f32(int64_t n_rows, int32_t d, const int32_t *row_ptr, const int32_t *col_idx,
                       const float *val, const float *X, int64_t ldx, float *Y, int64_t ldy,
                       int accumulate, void *stream);

/*
 * The whole aggregation loop of CoreDiffusion.forward, layers.py:41-48, plus the
 * stack/transpose of layers.py:58, in ONE pass over the edge list:
 *     res_0 = A_0·X (+ X if SELF_LOOP);  res_j = res_{j-1} + A_j·X;  H[:, j, :] = relu?(res_j)
 * The K matrices are given as one CSR whose entries carry a slot tag and are sorted by
 * (row, slot, col):  NESTED: entry tagged s is present in A_s, A_{s+1}, ..., A_{K-1};
 * otherwise it is present in A_s only.  H is [n_rows, K, d] contiguous (the [batch, core, feat]
 * layout nn.GRU(batch_first=True) consumes at layers.py:59).   1 <= K <= CTGCN_MAX_SLOTS.
 * long_rows (optional, device int32[n_long]): the rows with more than long_threshold entries (hubs).  They are
 * skipped by the row-per-lane-group kernel and processed one 1024-thread block each, so that a 100k-entry row does
 * not serialise on 32 lanes.  n_long == 0 disables the split.
 * hub_split > 1 with a hub workspace (ctgcn_hub_workspace_bytes(n_long, hub_split, slots = K forward / 1 backward, d) bytes, 16-byte
 * aligned): a hub row of L entries is cut into min(hub_split, ceil(L / 8192)) pieces, one block each; a second small kernel adds the
 * pieces' partial sums in piece order and finishes the row (two passes, fixed order: results do not depend on scheduling).
 * hub_split <= 1 or a NULL workspace: one block per hub row.  hub_split <= 64.
 */
size_t ctgcn_hub_workspace_bytes(int32_t n_long, int32_t hub_split, int32_t slots, int32_t d);
/* entries per piece when a hub row is cut (the 8192 above): callers derive hub_split = ceil(longest row / this) from it */
int32_t ctgcn_hub_split_entries(void);
int ctgcn_core_aggregate_f32(int64_t n_rows, int32_t d, int32_t K, const int32_t *row_ptr,
                             const int32_t *col_idx, const float *val, const uint8_t *slot,
                             const float *X, int64_t ldx, float *H, uint32_t flags,
                             const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                             int32_t hub_split, void *hub_workspace, size_t hub_workspace_bytes, void *stream);
/*
 * The same aggregation over the rows of Linear(one-hot features) = W^T + b (layers.py:95-106 on helper.py:161-172) without that matrix:
 * Wt is the Linear's weight stored by input row, [n_rows, d] dense (row stride d), and every operand row the kernels read - a gathered
 * neighbour row or the row's own self-loop row - is Wt[row] + gather_bias as ONE fp32 add in registers before the multiply-accumulate:
 * the value a materialised W^T + b would have held, so H is bit-identical to ctgcn_core_aggregate_f32 on that matrix (hub rows and
 * hub rows cut into pieces included).  gather_bias: float[d] or NULL (NULL: ctgcn_core_aggregate_f32 with ldx = d).
 */
int ctgcn_core_aggregate_bias_f32(int64_t n_rows, int32_t d, int32_t K, const int32_t *row_ptr,
                                  const int32_t *col_idx, const float *val, const uint8_t *slot,
                                  const float *Wt, const float *gather_bias, float *H, uint32_t flags,
                                  const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                                  int32_t hub_split, void *hub_workspace, size_t hub_workspace_bytes, void *stream);

/*
 * Backward of ctgcn_core_aggregate_f32 w.r.t. X (what autograd derives for layers.py:41-48).
 * Step 1 (ctgcn_core_aggregate_bwd_prep_f32), elementwise over [n, K, d]:
 *     G_j = dH_j * [H_j > 0] (RELU) ; S_j = sum_{i>=j} G_i ; Z_j = NESTED ? sum_{i>=j} S_i : S_j
 *     S0 = S_0  ([n, d], the self-loop term; may be NULL when SELF_LOOP is not set)
 * Step 2 (ctgcn_core_aggregate_bwd_f32) on the CSR of the TRANSPOSED matrices (same arrays when
 * the adjacency is symmetric, which every matrix the reference loader builds is):
 *     dX[r] = S0[r] (SELF_LOOP) + sum_{e in row r} val[e] * Z[col[e], slot[e], :]
 */
int ctgcn_core_aggregate_bwd_prep_f32(int64_t n_rows, int32_t d, int32_t K, const float *dH,
                                      const float *H, float *Z, float *S0, uint32_t flags,
                                      void *stream);
int ctgcn_core_aggregate_bwd_f32(int64_t n_rows, int32_t d, int32_t K, const int32_t *row_ptr,
                                 const int32_t *col_idx, const float *val, const uint8_t *slot,
                                 const float *Z, const float *S0, float *dX, int64_t lddx,
                                 uint32_t flags, const int32_t *long_rows, int32_t n_long,
                                 int32_t long_threshold, int32_t hub_split, void *hub_workspace, size_t hub_workspace_bytes,
                                 void *stream);

/*
 * Edge rows (in file order) -> the snapshot's simple undirected weighted graph as symmetric, zero-diagonal CSR
 * with sorted columns.  Replaces the graph construction at utils.py:23-30 (get_nx_graph) and utils.py:35-58
 * (get_sp_adj_mat): every row sets weight({src,dst}) = w (1.0 when w == NULL); the LAST row naming an
 * unordered pair wins; rows with src == dst are dropped.  src/dst: int32[m] node indices in [0, n).
 * Outputs: row_ptr int32[n+1]; col_idx int32 / val float with capacity 2*m; *nnz_host = entries stored
 * (2 x distinct pairs).  workspace: ctgcn_workspace_bytes(CTGCN_OP_INGEST, n, m, 0, 0).  Synchronises `stream`.
 */
int ctgcn_edges_to_csr(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w,
                       int32_t *row_ptr, int32_t *col_idx, float *val, int64_t *nnz_host,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Core number of every vertex of an undirected simple graph given as symmetric CSR structure
 * (self-loop entries, if any, are ignored).  Replaces networkx.core_number at
 * preprocessing/structure_generation.py:35.  Integer result, unique, bit-exact.
 * workspace: ctgcn_workspace_bytes(CTGCN_OP_KCORE, n, nnz, 0, 0) bytes.
 * level_cap <= 0: exact core numbers.  level_cap = L > 0: only levels 0..L-1 are peeled and every vertex whose core
 * number is >= L is reported as L — all a loader with max_core = L needs (helper.py:63 keeps k <= max_core, so the
 * levels above it are never told apart), at a fraction of the peel depth.
 * max_core_host (optional) receives max(core) (capped likewise).  Synchronises `stream`.
 */
int ctgcn_kcore_i32(int64_t n, const int32_t *row_ptr, const int32_t *col_idx, int32_t *core,
                    void *workspace, size_t workspace_bytes, int32_t level_cap, int32_t *max_core_host,
                    void *stream);

/*
 * level[e] = min(core[row(e)], core[col(e)]) for every CSR entry: entry e belongs to the k-core
 * subgraph A_k (structure_generation.py:48-53, networkx.k_core) iff level[e] >= k.
 * Also accumulates, for L in [0, hist_len): count[L] = #entries with min(level, hist_len-1) == L
 * and wsum[L] = sum of their weights (fp64) — what helper.py:74-75 needs to decide
 * `delta.sum() == 0`.  count/wsum must be zeroed by the caller; either may be NULL.
 */
int ctgcn_edge_levels_i32(int64_t n, const int32_t *row_ptr, const int32_t *col_idx,
                          const float *val, const int32_t *core, int32_t *level,
                          int64_t *count, double *wsum, int32_t hist_len, void *stream);

/*
 * Tag every entry with its slot (slot_of_level[min(level, table_len-1)], table of uint8 on the
 * device) and stably re-order the entries of each row by slot, producing the (row, slot, col)
 * order ctgcn_core_aggregate_f32 consumes.  Encodes helper.py:63-78 (file truncation, reversal,
 * skipped matrices) once the caller has built the table.  Outputs must not alias inputs.
 */
int ctgcn_slot_reorder(int64_t n, int32_t K, const int32_t *row_ptr, const int32_t *col_idx,
                       const float *val, const int32_t *level, const uint8_t *slot_of_level,
                       int32_t table_len, int32_t *col_out, float *val_out, uint8_t *slot_out,
                       void *stream);

/*
 * Recurrent part of a single-layer GRU over `steps` for `rows` independent sequences, hidden = 128,
 * fused with the reduction the reference applies to its output:
 *   reduce_sum != 0 :  out[rows,128]        = LayerNorm(sum_t h_t)   nn.GRU + .sum(dim=1) + LayerNorm, layers.py:59-62
 *   reduce_sum == 0 :  out[rows,steps,128]  = LayerNorm(h_t)         nn.GRU + LayerNorm, models.py:249-250
 * gi [rows, steps, 384] is the input projection x·W_ih^T + b_ih (+ b_hh for the r and z gates) in PyTorch's
 * gate order r,z,n — a plain GEMM the caller runs with its BLAS; w_hh [384,128] and b_hn [128] (the n-gate's
 * hidden bias, NULL = 0) are the module's weight_hh_l0 and bias_hh_l0[256:384].  ln_weight == NULL skips the
 * LayerNorm.  h_0 = 0.  split_bf16 selects the arithmetic of the product h_{t-1}·W_hh^T (all fp32-accurate, fp32 I/O):
 *   CTGCN_SPLIT_NONE   (0)  f32-input MFMA (an fmaf chain)
 *   CTGCN_SPLIT_BF16X3 (1)  operands split exactly into three bf16 terms, six partial products, fp32 accumulation
 *   CTGCN_SPLIT_F16X2  (2)  operands scaled per row by a power of two and split into two fp16 terms (22 bits), three
 *                           partial products, fp32 accumulation: half the matrix-core work of (1) and measured MORE
 *                           accurate than (0) and (1) (tools/probes/mfma_f16x2_probe.hip)
 * ld_out (reduce_sum only; 0 = dense 128): floats between output rows — lets a snapshot's embeddings land directly in
 *   column t of the [nodes, T, 128] input of the temporal GRU (models.py:248 stack + transpose without the copies).
 * gi_blocked != 0 (CTGCN_SPLIT_F16X2 only): gi is in the tile layout ctgcn_gru_input_proj_f32 writes for steps_blocked = steps
 *   ([node tile of 64][step][gate][16-column group][node in tile][16]; the buffer must cover ceil(rows/64)*64 rows).
 * gates_out (optional; requires reduce_sum == 0 and ln_weight == NULL): [rows, steps, 4, 128] receives r, z, n and
 * q = W_hn·h_{t-1} + b_hn for ctgcn_gru_seq_bwd_f32.
 * row_order / tile_mask / tile_base (all or none; reduce_sum, CTGCN_SPLIT_F16X2, plain gi layout, steps <= 64): gi was projected from
 * the COMPACT operand rows ctgcn_core_aggregate_split_f32 wrote under a row plan with tiles of 64 — only the steps that bring a new x
 * row exist: tile T starts at gi row tile_base[T], sequence p of it owns popcount(tile_mask[T]) consecutive rows, step t reads the row of
 * the last set bit <= t.  Sequence p is written to out row row_order[p].  Same arithmetic on the same numbers: bit-identical.
 */
int ctgcn_gru_seq_f32(int64_t rows, int32_t steps, int32_t hidden, const float *gi, const float *w_hh,
                      const float *b_hn, const float *ln_weight, const float *ln_bias, float ln_eps,
                      int reduce_sum, float *out, int64_t ld_out, float *gates_out, int split_bf16, int gi_blocked,
                      const int32_t *row_order, const uint32_t *tile_mask, const int32_t *tile_base, void *stream);

/*
 * Backward of the LayerNorm(128) behind the GRU (layers.py:61-62 norm(output.sum(dim=1)); models.py:250 norm(output)):
 *   x[r] = sum_{t < steps} h[r, t, :]  (steps = 1: h is [rows, 128]);  dx = dL/dx given dy = dL/dLayerNorm(x) (the mean / rstd are recomputed),
 *   partial [n_partial, 256]: per-block partial sums of (dgamma | dbeta), every row written; the caller adds them up (deterministic).
 *   ld_dy: floats between the rows of dy (0 = 128; larger: dy is a column of a [rows, T, 128] gradient, no copy needed).
 * One pass instead of the framework's three kernels + sum + forward recompute.  n_partial = number of blocks (<= 65535, e.g. 2048).
 *   dy_rows (optional, device int32[rows]): row p of h / dx belongs to row dy_rows[p] of dy (the GRU ran in a row-plan order).
 */
int ctgcn_layernorm_bwd_f32(int64_t rows, int32_t steps, int32_t hidden, const float *h, const float *dy, int64_t ld_dy, const float *gamma, float eps,
                            float *dx, float *partial, int32_t n_partial, const int32_t *dy_rows, void *stream);

/*
 * The same for nn.LSTM (rnn_type = 'LSTM'; layers.py:27-28, models.py:234-235): gi [rows, steps, 512] = x·W_ih^T + b_ih
 * + b_hh in PyTorch's gate order i,f,g,o; w_hh [512, 128]; h_0 = c_0 = 0.  Exact fp32 (f32-input MFMA).
 * gates_out (optional; reduce_sum == 0, no LayerNorm): [rows, steps, 5, 128] for ctgcn_lstm_seq_bwd_f32 (training's recompute pass).
 */
int ctgcn_lstm_seq_f32(int64_t rows, int32_t steps, int32_t hidden, const float *gi, const float *w_hh,
                       const float *ln_weight, const float *ln_bias, float ln_eps, int reduce_sum, float *out,
                       float *gates_out, void *stream);
/*
 * Backward of that recurrence (autograd of nn.LSTM).  gates [rows, steps, 5, 128] = i, f, g, o (after their activations) and c, as
 * ctgcn_lstm_seq_f32 writes them into gates_out (reduce_sum == 0, no LayerNorm: `out` is then the raw h sequence).  dh_seq
 * [rows, steps, 128] and / or dh_sum [rows, 128] (added at every step: the gradient of sum_t h_t).  d_gi [rows, steps, 512] = gradient
 * w.r.t. the gate pre-activations (= d of x·W_ih^T + b; d x, d W_ih, d W_hh are GEMMs over it), bias_partial [n_partial, 512]: per-block
 * column sums of d_gi (d b_ih = d b_hh = their sum).  Exact fp32 (f32-input MFMA).
 */
int ctgcn_lstm_seq_bwd_f32(int64_t rows, int32_t steps, int32_t hidden, const float *gates, const float *dh_seq, const float *dh_sum,
                           const float *w_hh, float *d_gi, float *bias_partial, int32_t n_partial, void *stream);

/*
 * layers.py:59-62 / models.py:249-250 in ONE kernel for d_in = hidden = 128 with both weight matrices resident in the register
 * file of the CU (four waves, one per SIMD, 512 registers each): the input projection gi is consumed from the MFMA accumulators
 * and never materialised - not in HBM, not in a workspace.  x [rows, steps, 128] with row-step stride ldx.
 *   reduce_sum != 0: out[rows, ld_out] = LayerNorm(sum_t h_t) (ld_out as in ctgcn_gru_seq_f32, 0 = dense 128)
 *   reduce_sum == 0: out[rows, steps, 128] = LayerNorm(h_t) per step (ld_out must be 0)
 * ln_weight / ln_bias NULL: no LayerNorm.  bias_gi [384] = b_ih (+ b_hh for the r and z gates), b_hn [128] = bias_hh_l0[256:384];
 * either may be NULL.  CTGCN_SPLIT_F16X2 arithmetic, operation for operation that of ctgcn_gru_input_proj_f32 followed by
 * ctgcn_gru_seq_f32: results are bit-identical to the kernel pair.  HBM traffic: x in + out (the pair: 7x that).
 * gates_out (optional; reduce_sum == 0, no LayerNorm): [rows, steps, 4, 128] as ctgcn_gru_seq_f32 writes them - the recompute pass of
 * training without the gi round trip.
 * step_offsets (optional, device int64[steps]) + ld_row: x of step t of sequence r is read at x + r ld_row + step_offsets[t] (floats;
 * offsets multiples of 4) instead of x + (r steps + t) ldx - the steps of a sequence may live in different buffers' regions (the temporal
 * GRU of models.py:249 on the receive buffer of a snapshot-parallel exchange, no stack / transpose copy).  At most 32 steps with
 * step_offsets: longer tables return CTGCN_E_UNSUPPORTED (the caller gathers such sequences into a dense x first).
 */
int ctgcn_gru_layer_f32(int64_t rows, int32_t steps, int32_t d_in, int32_t hidden, const float *x, int64_t ldx, const float *w_ih,
                        const float *w_hh, const float *bias_gi, const float *b_hn, const float *ln_weight, const float *ln_bias,
                        float ln_eps, int reduce_sum, float *out, int64_t ld_out, float *gates_out,
                        const int64_t *step_offsets, int64_t ld_row, void *stream);

/*
 * ctgcn_gru_layer_f32 (sum-over-steps form) on an input that ctgcn_core_aggregate_split_f32 already wrote as fp16 planes + row scales
 * (d = hidden = 128: `planes` = that call's workspace for n_rows = rows, K = steps).  The aggregation (HBM-bound) does the per-row
 * max / scale / split, this matrix-core-bound kernel only copies the planes into LDS: the whole CoreDiffusion layer of
 * layers.py:41-62 in two kernels, x [rows, steps, 128] never exists in fp32.  Bit-identical to ctgcn_core_aggregate_f32 +
 * ctgcn_gru_layer_f32.  Inference only.
 *   row_order / tile_mask (both or neither; steps <= 64): the row plan the aggregation call was given (see there).  Sequence p of the
 *   planes is written to out row row_order[p]; a step whose tile_mask bit is clear re-uses the x·W_ih products of the step before
 *   (its x row is the same row again: layers.py:41-48 with no entry of that slot or below in any of the tile's 16 rows) and costs the
 *   h·W_hh half only.  Same products in the same order: results are bit-identical to the call without a plan.
 */
int ctgcn_gru_layer_presplit_f32(int64_t rows, int32_t steps, int32_t hidden, const void *planes, const float *w_ih, const float *w_hh,
                                 const float *bias_gi, const float *b_hn, const float *ln_weight, const float *ln_bias, float ln_eps,
                                 float *out, int64_t ld_out, const int32_t *row_order, const uint32_t *tile_mask, void *stream);

/*
 * Training under the row plan (round 4): the backward of a CoreDiffusion layer with d_in = hidden = 128 (layers.py:41-62; what
 * embedding.py:347-348 runs every batch) in position order, chunk by chunk, with two intermediates in HBM instead of six.
 *
 * ctgcn_gru_layer_presplit_save_f32 — the recompute pass: ctgcn_gru_layer_presplit_f32's kernel on the sequences
 *   [first_row, first_row + rows) of the forward's planes (`planes`, plane_rows = n K rows per plane; first_row a multiple of 16;
 *   tile_mask, optional, already points at tile first_row / 16), writing the gates [rows, steps, 4, 128] (r, z, n, q = W_hn h + b_hn), the
 *   raw h sequence [rows, steps, 128] and the pre-LayerNorm sum over the steps [rows, 128] — no LayerNorm, no `out`.  Its gates are
 *   [rows, steps, 3, 128] = r, z, q (gate_count = 3 below): n is rebuilt from h_t, h_{t-1} and z, h_t = n + z (h_{t-1} - n).
 * ctgcn_gru_bwd_rec_f32 — backward recurrence + dW_hh: gates (gate_count = 4: r, z, n, q as ctgcn_gru_layer_f32 / ctgcn_gru_seq_f32 write them; 3: r, z, q), h_seq as above; exactly one of dh_sum [rows, 128] (gradient of sum_t h_t,
 *   added at every step) / dh_seq [rows, steps, 128]; d_gi [rows, steps, 384] receives, at every step whose tile_mask bit is set, the sum
 *   of (da_r, da_z, da_n) over that step and the steps after it that repeat its x (tile_mask NULL: every step);
 *   dw_partial [n_partial, 384, 128] / dbn_partial [n_partial, 128]: per-block sums of dW_hh and of the n-gate column of d b_hh
 *   (n_partial >= ctgcn_gru_bwd_blocks(rows), rows of the tables beyond that are not touched; accumulate != 0 adds to them: zero the
 *   tables once, accumulate over the chunks, one reduction at the end — deterministic).
 *   bf16 x 2 split arithmetic (three v_mfma_f32_16x16x32_bf16 per product).
 *   steps <= 64 for the three calls of this block (round 6; 32 before): tile_mask holds one word per 16-row tile up to 32 steps and two
 *   (steps 0-31, 32-63; tile t at [2 t], [2 t + 1]) beyond, as the forward's row plan does — core lists of 33-64 matrices (America-Air /
 *   Europe-Air depth) train under the plan too.
 *   Precondition of both calls below (not checked): bit 0 of every tile's mask is set — step 0 is always fresh; it is the unit that
 *   closes a tile (the last d_gi sum is written there, the Z / S0 epilogue ends there).  Bits at and above `steps` are ignored, in the
 *   one-word and in the two-word form.  Both calls must be given the same masks.
 * ctgcn_gru_bwd_in_f32 — dx = d_gi·W_ih, dW_ih, d b_ih over the fresh steps: x either as the forward's planes (x_planes, plane_rows,
 *   first_row as above) or fp32 rows (x, row-step stride ldx).  Output either dx [rows, steps, 128] or (Z != NULL) the aggregation
 *   backward's operands in matrix-row order: Z [n, steps, 128] and S0 [n, 128] (NULL without self loop) with the ReLU mask x > 0 and
 *   the suffix sums of ctgcn_core_aggregate_bwd_prep_f32 applied (nested: CTGCN_F_NESTED lists), written at row row_order[p]
 *   (row_order points at first_row; NULL: p).  Z is only defined at fresh steps — a row has no entry tagged with a step that
 *   repeats, ctgcn_core_aggregate_bwd_f32 never reads the others (symmetric lists).
 */
int32_t ctgcn_gru_bwd_blocks(int64_t rows);
int ctgcn_gru_layer_presplit_save_f32(int64_t rows, int32_t steps, int32_t hidden, const void *planes, int64_t plane_rows, int64_t first_row,
                                      const float *w_ih, const float *w_hh, const float *bias_gi, const float *b_hn, const uint32_t *tile_mask,
                                      float *gates_out, float *hseq_out, float *presum_out, void *stream);
int ctgcn_gru_bwd_rec_f32(int64_t rows, int32_t steps, int32_t hidden, const float *gates, int32_t gate_count, const float *h_seq, const float *dh_sum,
                          const float *dh_seq, const float *w_hh, const uint32_t *tile_mask, float *d_gi, float *dw_partial,
                          float *dbn_partial, int32_t n_partial, int32_t accumulate, void *stream);
int ctgcn_gru_bwd_in_f32(int64_t rows, int32_t steps, int32_t hidden, const float *d_gi, const float *w_ih, const uint32_t *tile_mask,
                         const void *x_planes, int64_t plane_rows, int64_t first_row, const float *x, int64_t ldx, float *dx, float *Z, float *S0,
                         const int32_t *row_order, int32_t nested, float *dw_partial, float *dbi_partial, int32_t n_partial,
                         int32_t accumulate, void *stream);

/*
 * One launch per kernel for a whole WINDOW of small snapshots (reference models.py:243-247 loops over the snapshots; at 6 828 - 87 036 nodes a
 * snapshot's aggregation is 25 - 200 us of kernel, mostly ramp, tail and dependent load chains): the width-128 CoreDiffusion layer of `groups`
 * snapshots that share the node set (n_rows each), every snapshot with its own graph, inputs, weights and outputs.
 *   ctgcn_core_aggregate_split_group_f32   = ctgcn_core_aggregate_split_f32(d = 128, n_out = 1, no hub rows) per group, one grid
 *   ctgcn_gru_layer_presplit_group_f32     = ctgcn_gru_layer_presplit_f32 per group, one persistent grid of <= one block per CU: a block serves
 *                                            one snapshot (its weights stay resident), blocks are dealt out in proportion to `work`
 * Same kernels' code per snapshot: bit-identical to the per-snapshot calls.  g: HOST array of `groups` descriptors; table: device memory,
 * 256-byte aligned, ctgcn_group_table_bytes(groups) bytes, that the call fills on `stream` before the launch (do not reuse it for
 * another call before that call's kernel has run — same stream: fine).  Hub rows (longer than the caller's long-row threshold) are not
 * handled here: windows that have any take the per-snapshot calls.
 *
 * How the table is filled (ABI 28; rounds 4-5 used hipMemcpyAsync from pageable memory: a host stall per call, not capturable): the descriptor
 * bytes travel as kernel arguments of a small writer kernel — asynchronous, stream-ordered, recordable into a hipGraph, no host-to-device copy.
 * `shadow` (all ctgcn_*_group_f32 calls; may be NULL): HOST memory of the table's size that the caller zero-fills once and keeps together with
 * `table`.  The call compares this call's descriptors with the shadow; when they are equal the device table is current and NOTHING is written
 * (the steady state of an inference loop over one window: same graphs, weights and buffers forward after forward); otherwise table and shadow
 * are rewritten.  A caller that passes a shadow promises that nothing else writes to `table`, and that it always uses the pair on the same
 * stream (the table's last writer and its readers must be stream-ordered).  One (table, shadow) pair per call site: two calls sharing a table
 * would rewrite it every time.
 */
typedef struct {
    const int32_t *row_ptr, *col_idx;
    const float *val;
    const uint8_t *slot;
    const float *X;
    int64_t ldx;
    int32_t K;
    uint32_t flags;
    const int32_t *row_order;      /* row plan (both or neither), as ctgcn_core_aggregate_split_f32 */
    const uint32_t *tile_mask;
    void *workspace;               /* d = 128, consumer = the GRU layer kernel: planes + row scales of the group,
                                      ctgcn_core_aggregate_split_workspace_bytes(n_rows, 128, K, 1, 0) bytes, 256-byte aligned (planes1 = NULL) */
    size_t workspace_bytes;
    /* consumer = the split GEMM (round 5: the 500-wide first layer, any d <= 512): the group's operand rows inside planes SHARED by the window —
     * pointers to the group's first row of plane 1 / plane 2 (row length = d rounded up to 64 halfs) and of the scales; with a row plan the
     * rows are compact (tile 64) and tile_base gives each tile's first row RELATIVE to the group's first row */
    void *planes1, *planes2;
    float *scales;
    const int32_t *tile_base;
} ctgcn_agg_split_group_t;
typedef struct {
    const void *planes;            /* the group's aggregation workspace */
    const float *w_ih, *w_hh, *bias_gi, *b_hn, *ln_weight, *ln_bias;
    float ln_eps;
    int32_t steps;                 /* K of the snapshot */
    float *out;
    int64_t ld_out;
    const int32_t *row_order;
    const uint32_t *tile_mask;
    int64_t work;                  /* relative cost (e.g. (position, step) rows that bring a new x + rows x steps); <= 0: equal shares */
} ctgcn_gru_layer_group_t;
typedef struct {
    const float *gi;               /* gate pre-activations of the group's (compact) operand rows, [rows, 384] */
    const float *w_hh, *b_hn, *ln_weight, *ln_bias;
    float ln_eps;
    int32_t steps;
    float *out;
    int64_t ld_out;
    const int32_t *row_order;      /* the aggregation's row plan (tile 64): all three or none */
    const uint32_t *tile_mask;
    const int32_t *tile_base;
    int64_t work;
} ctgcn_gru_seq_group_t;
size_t ctgcn_group_table_bytes(int32_t groups);
/* Diagnostic: descriptor tables written by the grouped calls of this process so far (current = 0), or found current through their shadow and
 * not written (current = 1).  A steady-state inference loop moves only the second counter (tests/test_gpu_group.py). */
uint64_t ctgcn_table_uploads(int current);
/* Round 5, the 500-wide first CoreDiffusion layer of a small window in one launch per kernel (reference models.py:243-247 loops over the
 * snapshots): Linear(I) = W^T + b of every snapshot; the aggregation into shared operand planes (ctgcn_agg_split_group_t, GEMM form);
 * ctgcn_linear_packed_group_f32 (one panel GEMM over all snapshots' rows, weights per snapshot); the recurrences. */
int ctgcn_transpose_bias_group_f32(int32_t groups, int64_t n, int32_t d, const float *const *w, int64_t ldw, const float *const *bias, float *const *out,
                                   int64_t ldo, void *table, size_t table_bytes, void *shadow, void *stream);
int ctgcn_gru_seq_group_f32(int32_t groups, int64_t rows, int32_t hidden, const ctgcn_gru_seq_group_t *g, void *table, size_t table_bytes, void *shadow,
                            void *stream);
int ctgcn_core_aggregate_split_group_f32(int32_t groups, int64_t n_rows, int32_t d, const ctgcn_agg_split_group_t *g, void *table, size_t table_bytes,
                                         void *shadow, void *stream);
int ctgcn_gru_layer_presplit_group_f32(int32_t groups, int64_t rows, int32_t hidden, const ctgcn_gru_layer_group_t *g, void *table, size_t table_bytes,
                                       void *shadow, void *stream);

/*
 * Dense  y[rows, n_out] = x[rows, k]·w[n_out, k]^T + bias  (bias [n_out] may be NULL) in fp32-accurate fp16x2 split arithmetic on the
 * matrix cores (CTGCN_SPLIT_F16X2: operand rows scaled by a power of two and written as two fp16 terms, three
 * v_mfma_f32_16x16x32_f16 per product, fp32 accumulation) - the GRU input projection for d_in != 128 (layers.py:59 with
 * input_size = hid_dim = 500) and nn.Linear on dense inputs (layers.py:95-106), which otherwise run as fp32 library GEMMs.
 * ldx / ldw / ldy: row strides in floats.  Any k >= 1 (rows that are only 4-byte aligned, e.g. k = 1737, are read with the same 16-byte
 * loads), any n_out (more than 512 columns: one launch per 512).  activation: CTGCN_ACT_NONE, or CTGCN_ACT_SELU applied to y in the
 * epilogue (the F.selu after each Linear of an 'N' MLP).
 * workspace: ctgcn_linear_workspace_bytes(rows, n_out, k) bytes, 256-byte aligned: ctgcn_split_planes_bytes(rows, k) bytes of x's operand
 * planes followed by ctgcn_pack_weight_bytes(n_out, k) bytes of w's packed operand.
 */
size_t ctgcn_linear_workspace_bytes(int64_t rows, int32_t n_out, int32_t k);
/*
 * The same product with the operands kept by the caller: an operand that does not change between calls — the weights of an inference run,
 * node features the reference builds once and feeds to every batch (train.py:72-76) — is prepared ONCE:
 *   ctgcn_split_rows_f32      x side: rows x k fp32 (row stride ldx) -> `planes`: plane 1 [rows, kp] | plane 2 | row scales, kp = k rounded up
 *                             to 64 (zero padded), ctgcn_split_planes_bytes(rows, k) bytes, 256-byte aligned
 *   ctgcn_pack_weight_f32     w side (round 5): n_out x k fp32 (row stride ldw) -> `packed`: the same split stored in matrix-core fragment order
 *                             ([column tile of 16][k slab of 32][plane][lane][8 halfs], column tiles padded to a multiple of 8 per chunk of 512
 *                             columns) | column scales; ctgcn_pack_weight_bytes(n_out, k) bytes, 256-byte aligned
 *   ctgcn_linear_packed_f32   y = x·w^T + bias (+ activation) from x's planes and w's packed operand (gemm_h2_panel_kernel: persistent blocks,
 *                             each 128-row panel of x read once over the full width)
 * Same split, same kernel as ctgcn_linear_f32: bit-identical results.
 */
size_t ctgcn_split_planes_bytes(int64_t rows, int32_t k);
size_t ctgcn_pack_weight_bytes(int32_t n_out, int32_t k);
int ctgcn_split_rows_f32(int64_t rows, int32_t k, const float *x, int64_t ldx, void *planes, size_t planes_bytes, void *stream);
int ctgcn_pack_weight_f32(int32_t n_out, int32_t k, const float *w, int64_t ldw, void *packed, size_t packed_bytes, void *stream);
int ctgcn_linear_packed_f32(int64_t rows, int32_t n_out, int32_t k, const void *x_planes, const void *w_packed, const float *bias,
                            int32_t activation, float *y, int64_t ldy, void *stream);
/* ctgcn_linear_packed_f32 whose output leaves as the NEXT layer's X operand (the hidden layers of the MLP, reference layers.py:95-106, in
 * inference): out_planes = what ctgcn_split_rows_f32(rows, n_out, y) would write for y = act(x w^T + bias) — per-row scale + two fp16 planes
 * [rows, n_out rounded up to 64], bit for bit — without y going to memory as fp32 and coming back.  n_out <= 512;
 * out_planes: ctgcn_split_planes_bytes(rows, n_out) bytes, 256-byte aligned. */
int ctgcn_linear_packed_chain_f32(int64_t rows, int32_t n_out, int32_t k, const void *x_planes, const void *w_packed, const float *bias, int32_t activation,
                                  void *out_planes, size_t out_planes_bytes, void *stream);
/* ctgcn_linear_packed_f32 for the operand rows of `groups` snapshots in ONE launch (the 500-wide first layer of a small window): planes1 /
 * planes2 / scales / y hold the rows of all groups one after the other, every group padded to whole panels of 128 rows (total_rows % 128 == 0;
 * rows a group does not fill are multiplied and written like any other: give them finite contents or ignore them); panel_group (DEVICE,
 * total_rows / 128 entries) names the group of every panel; w_packed[i] / bias[i] (host arrays of device pointers): the group's packed weight
 * and bias.  n_out <= 512.  table / shadow: as for the other grouped calls above (256-byte aligned device memory, >= 24 bytes per group —
 * ctgcn_group_table_bytes covers it; optional host shadow of the same size).  Same arithmetic per row as ctgcn_linear_packed_f32: bit-identical to the per-group calls. */
int ctgcn_linear_packed_group_f32(int32_t groups, int64_t total_rows, int32_t n_out, int32_t k, const void *planes1, const void *planes2,
                                  const float *scales, const int32_t *panel_group, const void *const *w_packed, const float *const *bias,
                                  int32_t activation, float *y, int64_t ldy, void *table, size_t table_bytes, void *shadow, void *stream);
int ctgcn_linear_f32(int64_t rows, int32_t n_out, int32_t k, const float *x, int64_t ldx, const float *w, int64_t ldw, const float *bias,
                     int32_t activation, float *y, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream);

/*
 * CoreDiffusion aggregation (ctgcn_core_aggregate_f32: layers.py:41-48,58) whose only consumer is the GRU input projection of a
 * layer with d_in != 128 (layers.py:59, nn.GRU(input_size = hid_dim = 500, ...)): instead of the fp32 H [n_rows, K, d] the kernel
 * writes what ctgcn_linear_f32 would make of it - the per-row scales and the two fp16 planes of the n_rows*K operand rows
 * (row = node*K + core) - straight into that GEMM's workspace, bit-identical to aggregate + ctgcn_linear_f32, without the
 * write + read + write of the fp32 intermediate.  Inference only (nothing is kept for a backward pass).
 *   d % 4 == 0, d <= 512, X 16-byte aligned, ldx % 4 == 0.  The same planes serve both consumers (one split
 *   definition: scale 2^(e-14), leading term fp16(x/s), residual fp16(x/s - leading)); at d = 128 that is ctgcn_gru_layer_presplit_f32.
 *   workspace: ctgcn_core_aggregate_split_workspace_bytes(n_rows, d, K, n_out, n_long) bytes, 256-byte aligned; n_out is the
 *   width of the projection that follows (its weight planes share the workspace); n_long hub rows pass through an fp32
 *   scratch at the end of it.
 * ctgcn_linear_presplit_f32(rows = n_rows*K, n_out, k = d, w, ...) then runs the GEMM on that workspace.
 *   Row plan (row_order, tile_mask: both or neither; K <= 64.  K <= 32: one mask word per tile; 33 <= K <= 64 (America-Air max core 64,
 *   Europe-Air 33): two, tile_mask[2 T] = slots 0-31, tile_mask[2 T + 1] = slots 32-63 - for every consumer of the same plan).
 *   A node whose first stored entry is tagged f has H[v, 0] = ... = H[v, f-1] = relu(x_v) (only the self loop has arrived): rows the
 *   reference computes, stacks and multiplies by W_ih f times (layers.py:41-48,58-59).  With a plan, operand rows p K .. p K + K - 1
 *   belong to matrix row row_order[p] (a permutation that puts rows with equal repeat patterns next to each other, so that the 16
 *   sequences of a GRU tile share one), and slot j of position p is only WRITTEN when bit j of tile_mask[p / 16] is set (bit 0 always
 *   is; a clear bit j promises that slot j repeats slot j - 1 for all 16 positions of the tile).  The planes' layout does not change -
 *   skipped rows are holes nobody reads.
 *   GEMM consumer (d != 128) under a row plan: tiles of 64 positions (the row tile of ctgcn_gru_seq_f32) and tile_base int32[tiles]:
 *   the operand rows are COMPACT - tile T's written rows start at row tile_base[T], position p owns popcount(tile_mask[T])
 *   consecutive rows (one per set bit, in slot order) from tile_base[T] + (p % 64) popcount(tile_mask[T]); operand_rows = their total
 *   (incl. the padding of the last tile), which is the row count ctgcn_linear_presplit_f32 is then called with, and
 *   ctgcn_gru_seq_f32 takes the same plan.  tile_base NULL with d = 128, n_out = 1.
 *   hub_row_dest int32[n_long K] (required under a row plan when n_long > 0): operand row of slot j of hub row long_rows[i], or -1
 *   when the plan does not want that slot.
 */
size_t ctgcn_core_aggregate_split_workspace_bytes(int64_t n_rows, int32_t d, int32_t K, int32_t n_out, int32_t n_long);
int ctgcn_core_aggregate_split_f32(int64_t n_rows, int32_t d, int32_t K, const int32_t *row_ptr, const int32_t *col_idx,
                                   const float *val, const uint8_t *slot, const float *X, int64_t ldx, uint32_t flags,
                                   const int32_t *long_rows, int32_t n_long, int32_t long_threshold, int32_t n_out,
                                   const int32_t *row_order, const uint32_t *tile_mask, const int32_t *tile_base, int64_t operand_rows,
                                   const int32_t *hub_row_dest,
                                   int32_t hub_split, void *hub_workspace, size_t hub_workspace_bytes,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* ctgcn_core_aggregate_split_f32 with operand rows Wt[row] + gather_bias (see ctgcn_core_aggregate_bias_f32): Wt [n_rows, d] dense,
 * gather_bias float[d], 16-byte aligned, or NULL; planes and row scales bit-identical to the call on the materialised W^T + b. */
int ctgcn_core_aggregate_split_bias_f32(int64_t n_rows, int32_t d, int32_t K, const int32_t *row_ptr, const int32_t *col_idx,
                                        const float *val, const uint8_t *slot, const float *Wt, const float *gather_bias, uint32_t flags,
                                        const int32_t *long_rows, int32_t n_long, int32_t long_threshold, int32_t n_out,
                                        const int32_t *row_order, const uint32_t *tile_mask, const int32_t *tile_base, int64_t operand_rows,
                                        const int32_t *hub_row_dest,
                                        int32_t hub_split, void *hub_workspace, size_t hub_workspace_bytes,
                                        void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_linear_presplit_f32(int64_t rows, int32_t n_out, int32_t k, const float *w, int64_t ldw, const float *bias, float *y, int64_t ldy,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of the recurrence above (autograd of nn.GRU, layers.py:59 / models.py:249).  Inputs: the saved gates and
 * the raw h sequence h_seq [rows, steps, 128]; the upstream gradient per step dh_seq [rows, steps, 128] and/or one
 * gradient dh_sum [rows, 128] added at every step (the .sum(dim=1) case).  Outputs, for the caller's GEMMs:
 *   d_gi  [rows, steps, 384] = dL/d(x·W_ih^T + b_ih)      -> dX = d_gi·W_ih, dW_ih = d_gi^T·x, db_ih = sum d_gi
 *   d_ghn [rows, steps, 128] = dL/d(W_hn·h + b_hn)         -> dW_hh = [d_gi_r, d_gi_z, d_ghn]^T·h_{t-1}, db_hh likewise
 * bias_partial (nullable) [n_partial, 512]: on return its rows sum to the bias gradients — columns 0..383 = sum over
 *   (row, step) of d_gi, columns 384..511 = of d_ghn (one row per launched block, the rest zeroed; n_partial >= the
 *   CU count uses the whole device).  Saves re-reading d_gi / d_ghn for db_ih / db_hh.
 * split_bf16: as in ctgcn_gru_seq_f32 (the product dGH·W_hh on the bf16 matrix cores, fp32-accurate).
 */
int ctgcn_gru_seq_bwd_f32(int64_t rows, int32_t steps, int32_t hidden, const float *gates, const float *h_seq,
                          const float *dh_seq, const float *dh_sum, const float *w_hh, float *d_gi, float *d_ghn,
                          float *bias_partial, int32_t n_partial, int split_bf16, void *stream);

/*
 * The GRU input projection  gi[rows, 384] = x[rows, 128]·w_ih^T + bias  (bias [384] may be NULL) for d_in = hidden = 128,
 * in fp32-accurate split arithmetic on the matrix cores: split_mode = CTGCN_SPLIT_BF16X3 or CTGCN_SPLIT_F16X2 (see
 * ctgcn_gru_seq_f32; error vs fp64 no larger than an fp32 fmaf chain's, measured).  Other widths: use a BLAS GEMM.
 * steps_blocked > 0 (CTGCN_SPLIT_F16X2 only): rows = nodes*steps_blocked rows of [nodes, steps, 128] sequences; gi is written
 * in the recurrence kernel's tile layout (see ctgcn_gru_seq_f32, gi_blocked) instead of [rows, 384].
 */
int ctgcn_gru_input_proj_f32(int64_t rows, int32_t d_in, int32_t hidden, const float *x, int64_t ldx,
                             const float *w_ih, const float *bias, float *gi, int split_mode, int32_t steps_blocked, void *stream);

/*
 * Gradient of the projection w.r.t. its input: d_x[rows, 128] = d_gi[rows, 384] · W_ih  (autograd of the F.linear inside
 * nn.GRU, reference layers.py:59), same split-bf16 arithmetic.  d_x rows are ldx floats apart.
 */
int ctgcn_gru_input_grad_f32(int64_t rows, int32_t d_in, int32_t hidden, const float *d_gi, const float *w_ih, float *d_x,
                             int64_t ldx, void *stream);

/*
 * Weight gradients of the GRU (autograd of nn.GRU's two F.linear, reference layers.py:59 / models.py:249):
 *   partial[p] (p < n_pairs), each [384, 128], sum over p = sum over r < rows of G[r, :]^T · X'[r, :]
 * G = gate columns [0,256) from g01 (row stride ldg01) and [256,384) from g2 (row stride ldg2): dW_ih takes both from
 * d_gi; dW_hh takes g2 = d_ghn.  X' = x (row stride ldx), or with shift_steps != 0 the rows shifted by one step inside
 * each `steps`-long sequence (X'[r] = r % steps ? x[r-1] : 0): h_{t-1} read straight from the h sequence.
 * accumulate != 0 adds to `partial` instead of overwriting it (one host-side sum after many calls).
 * rows = nodes * steps.  n_pairs: a positive multiple of 8 (half the CU count uses the whole device).  Split-bf16
 * arithmetic, deterministic.
 * Stride limit (CTGCN_E_UNSUPPORTED, nothing launched; ctgcn_last_error() names the operand and its largest usable ld): the kernel
 * reads each operand through one buffer descriptor per block — base = the block's first row, range clamped to 0x7fffffff bytes —
 * and 32-bit byte offsets.  Block pair p stages the 32-row chunks [p per, (p + 1) per), per = ceil(ceil(rows / 32) / n_pairs); the
 * shifted x is read from one row before the block's first (row - 1 of the matrix is never read).  With m the largest distance in
 * rows from a block's base to a row that holds data, (m ld + 32) · 4 <= 0x7fffffff must hold for ldg01, ldg2 and ldx alike (the
 * 32 is the column tail of the widest load); and when rows is no multiple of 32, the last staged row m' of the final chunk needs
 * (m' ld + 32) · 4 <= 2^32, so that its offset does not wrap back into the range and it reads as zero.  Full blocks have
 * m = 32 per - 1: a dense 384-wide d_gi with n_pairs = 8 reaches the limit at about 11 M rows, with the 128 pairs of an MI355X
 * at about 180 M; more pairs shorten the spans.
 */
int ctgcn_gru_weight_grad_f32(int64_t rows, int32_t steps, int32_t hidden, const float *g01, int64_t ldg01, const float *g2,
                              int64_t ldg2, const float *x, int64_t ldx, int shift_steps, float *partial, int32_t n_pairs,
                              int accumulate, void *stream);

/* Rows one wave of persistent blocks covers (rows per block x compute units): callers that split `rows` into
 * chunks should use multiples of this so that every launch keeps all CUs equally busy. */
int64_t ctgcn_gru_row_granule(void);
/* Compute units the persistent kernels run one block on (the device's, or the number set with ctgcn_set_persistent_cus): the grouped
 * launches take at most this many snapshots per call (ctgcn_gru_layer_presplit_group_f32 gives every snapshot at least one block). */
int32_t ctgcn_compute_units(void);

/*
 * Random-walk corpus (preprocessing/random_walk.py:8-69).  ctgcn_row_cumsum_f32: cumw[e] = inclusive prefix sum of the
 * weights within each CSR row.  ctgcn_random_walk_pairs: `walk_time` walks of walk_length steps from EVERY node (walk
 * indices first_walk .. first_walk+walk_time-1 of the seed's stream); next hop drawn with probability proportional to
 * the edge weight (weighted != 0) or uniformly; a walk stops at a node without neighbours.  For every walk the
 * (L+1)·L/2 position pairs i < j are written to pair_src/pair_dst (capacity n·walk_time·(L+1)·L/2; pairs with equal
 * endpoints or beyond the end of a short walk are written as the self pair (0,0), which ctgcn_edges_to_csr drops) and
 * freq[a]++, freq[b]++ (int64[n], caller-zeroed) for every emitted pair — the reference's node_freq_arr.
 * Feeding the pairs to ctgcn_edges_to_csr (w = NULL) yields the reference's symmetric 0/1 walk_spadj.
 */
int ctgcn_row_cumsum_f32(int64_t n, const int32_t *row_ptr, const float *val, float *cumw, void *stream);
int ctgcn_random_walk_pairs(int64_t n, const int32_t *row_ptr, const int32_t *col_idx, const float *cumw,
                            int32_t walk_length, int32_t walk_time, int32_t first_walk, uint64_t seed, int weighted,
                            int32_t *pair_src, int32_t *pair_dst, int64_t *freq, void *stream);

/*
 * Index draws of the negative-sampling loss (metrics.py:62-93).  For batch node b (batch_nodes[b], int64): all of its
 * walk partners (row of the pair CSR) if there are at most `num`, else `num` of them uniformly without replacement;
 * written at node_out/pos_out[offsets[b] ...] where offsets = exclusive scan of min(deg, num) (caller computes it).
 * neg_out[num]: the table entries at `num` distinct uniformly drawn positions of neg_table (random.sample semantics).
 * scratch: int64[num].
 */
int ctgcn_neg_sampling_indices(int64_t batch, const int64_t *batch_nodes, const int32_t *pair_row_ptr,
                               const int32_t *pair_col, int32_t num, int64_t table_len, const int32_t *neg_table,
                               uint64_t seed, const int64_t *offsets, int64_t *node_out, int64_t *pos_out,
                               int64_t *neg_out, int64_t *scratch, void *stream);

/*
 * One epoch of the reference's unsupervised schedule (embedding.py:330-368), per snapshot (ABI 29).  Positions p = 0..P-1 index the
 * epoch's node permutation perm (int64, distinct node ids); batch b holds positions [b*batch_size, min((b+1)*batch_size, P)), and there
 * are B = ceil(P / batch_size) batches.
 *
 * ctgcn_neg_sampling_offsets_batched: offsets[p] (int64[P+1]) = exclusive scan of min(deg(perm[p]), num) over the pair CSR, offsets[P]
 * = the total sample count (the one value a caller reads back to allocate); batch_offsets[b] (int64[B+1]) = offsets[b*batch_size],
 * batch_offsets[B] = the total.  workspace: ctgcn_epoch_scan_workspace_bytes(P).
 * ctgcn_neg_sampling_indices_batched: the draws of all batches; batch b's node / positive / negative indices are identical to what
 * ctgcn_neg_sampling_indices returns for that batch alone with seed seeds[b] (seeds: device uint64[B]).  Samples are laid out batch
 * after batch at node_out/pos_out[offsets[p] ...]; neg_out and scratch are int64[B, num].  node_out/pos_out may be NULL when
 * offsets[P] == 0.
 */
size_t ctgcn_epoch_scan_workspace_bytes(int64_t positions);
int ctgcn_neg_sampling_offsets_batched(int64_t positions, const int64_t *perm, const int32_t *pair_row_ptr, int32_t num,
                                       int64_t batch_size, int64_t *offsets, int64_t *batch_offsets, void *workspace,
                                       size_t workspace_bytes, void *stream);
int ctgcn_neg_sampling_indices_batched(int64_t positions, const int64_t *perm, int64_t batch_size, const uint64_t *seeds,
                                       const int32_t *pair_row_ptr, const int32_t *pair_col, int32_t num, int64_t table_len,
                                       const int32_t *neg_table, const int64_t *offsets, int64_t *node_out, int64_t *pos_out,
                                       int64_t *neg_out, int64_t *scratch, void *stream);

/*
 * The negative-sampling loss (metrics.py:38-66) of all B batches of one snapshot, forward and backward.  E: the snapshot's embeddings,
 * row v at E + v*lde (d <= 512).  With the outputs of the two calls above (`samples` = offsets[P]) and n_b the sample count of batch b:
 *   loss_out[b] = mean_s softplus(-e_u·e_v) + Q · mean_s softplus(e_u·S_b),  S_b = Σ_j E[neg[b, j]]   (double[B]; 0 when n_b = 0)
 * and dE (row v at dE + v*ldg) is ACCUMULATED with the gradient of Σ_b loss_b.  pos_sorted / pos_order: the positives pos_idx sorted
 * stably and the sample index of each; neg_sorted / neg_order: the same for the B*num flattened negatives.  Every row of dE is written
 * by one wave per kernel, no atomics: two calls give bit-identical dE.  workspace: ctgcn_negsampling_loss_workspace_bytes.
 */
size_t ctgcn_negsampling_loss_workspace_bytes(int64_t positions, int64_t samples, int64_t batch_size, int32_t d);
int ctgcn_negsampling_loss_fwd_bwd_f32(int64_t positions, int64_t batch_size, int64_t samples, int32_t d, int32_t num, float Q,
                                       const float *E, int64_t lde, const int64_t *offsets, const int64_t *node_idx,
                                       const int64_t *pos_idx, const int64_t *neg_idx, const int64_t *pos_sorted,
                                       const int64_t *pos_order, const int64_t *neg_sorted, const int64_t *neg_order,
                                       double *loss_out, float *dE, int64_t ldg, void *workspace, size_t workspace_bytes,
                                       void *stream);

/*
 * The reconstruction loss of CGCN-S / CTGCN-S (metrics.py:111-123) under the epoch partition, one snapshot: row r = rows[p] of batch b
 * has weight w = 1 / (|b| d); loss_out[b] = Σ_{p in b} w ||S[r] - E[r]||² (double[B]), and dS[r] += 2 w (S[r] - E[r]), dE[r] -= the
 * same (either gradient may be NULL).  rows must be distinct.  workspace: ctgcn_reconstruction_loss_workspace_bytes(P).
 */
size_t ctgcn_reconstruction_loss_workspace_bytes(int64_t positions);
int ctgcn_reconstruction_loss_fwd_bwd_f32(int64_t positions, int64_t batch_size, int32_t d, const int64_t *rows, const float *S,
                                          int64_t lds, const float *E, int64_t lde, double *loss_out, float *dS, int64_t ldds,
                                          float *dE, int64_t ldde, void *workspace, size_t workspace_bytes, void *stream);

/*
 * HOST function (no GPU work): write one snapshot's embedding [n, d] float32 (host pointer, leading dimension ld) as
 * the text file pandas produces for the reference's save_embedding, embedding.py:79-89
 * (pd.DataFrame(data, index=names).to_csv(path, sep=sep, header=True, index=True)), byte for byte: numpy float32
 * shortest-repr formatting, NaN as an empty field, minimal quoting of names.  names_blob_host holds the n
 * NUL-terminated node names, name_offsets_host[i] is the offset of name i.  threads <= 0: all host threads.
 */
int ctgcn_write_embedding_tsv(const char *path_host, int64_t n, int32_t d, const float *data_host, int64_t ld,
                              const char *names_blob_host, const int64_t *name_offsets_host, char sep,
                              int32_t threads);

/*
 * Link-prediction evaluation (evaluation/link_prediction.py; ctgcn_amd/evaluation/), ctgcn_eval.hip.
 *
 * ctgcn_lp_neg_sample: count negative edges (from_out[s], to_out[s]), s = 0..count-1, of a snapshot whose membership set is keys:
 * sorted unique int64 u*n_nodes + v, both directions of every edge.  Slot s draws uniform ordered pairs keyed on (seed, s, attempt)
 * until u != v and neither direction is in keys, so the output depends only on (seed, s).  A slot still without a pair after
 * max_attempts draws sets *flag (device int32) and the call returns CTGCN_E_LIMIT.  The call reads the flag back and therefore
 * synchronises `stream`.  n_nodes <= 3037000499 (keys fit in int64).
 *
 * The edge passes below evaluate `models` (<= 16) logistic-regression models on n edges (src[e], dst[e]) of the embedding E
 * (row v at E + v*lde, 1 <= d <= 256).  Model m uses the edge feature φ = measure_m(E[src], E[dst]), measure_m = bits 2m..2m+1 of
 * `measures` (0 Avg (a+b)/2, 1 Had a*b, 2 L1 |a-b|, 3 L2 (a-b)^2), and the parameters (w, b) = W[m*(d+1) .. +d], z = w·φ + b.
 * ctgcn_lp_grad_f32 and ctgcn_lp_scores_f32 take W as float[2, models, d+1]: hi then lo parts (W_hi + W_lo = the fp64 parameters;
 * lo may be zero), so z carries no systematic fp32 rounding of w.  ctgcn_lp_hess_f32 takes float[models, d+1].
 * Features are formed in registers and never stored.  label: uint8 {0,1}; s_e = w_pos or w_neg by label.  Node indices outside
 * [0, n_nodes) read as zero rows.  All reductions are per-block partials summed in a fixed order: repeated calls are bit-identical.
 *
 * ctgcn_lp_grad_f32: loss_out[m] = Σ_e s_e softplus(∓z) (double[models]), grad_out[m*(d+1) + j] = Σ_e s_e (σ(z_e) - y_e) φ̃_j with
 *   φ̃ = (φ, 1) (double[models, d+1]).  fp32 within a 32-edge tile, fp64 across tiles.  workspace: ctgcn_lp_grad_workspace_bytes.
 * ctgcn_lp_hess_f32: hess_out[m] = Σ_e s_e σ(1-σ) φ̃ φ̃ᵀ (double[models, d+1, d+1], symmetric); fp32 over parts of n/64 edges,
 *   fp64 across parts.  workspace: ctgcn_lp_hess_workspace_bytes.
 * ctgcn_lp_scores_f32: score_out[m*n + e] = z (float[models, n]).
 */
int ctgcn_lp_neg_sample(int64_t count, int64_t n_nodes, const int64_t *keys, int64_t n_keys, uint64_t seed, int64_t max_attempts,
                        int64_t *from_out, int64_t *to_out, int32_t *flag, void *stream);
size_t ctgcn_lp_grad_workspace_bytes(int64_t n, int32_t d, int32_t models);
int ctgcn_lp_grad_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                      const int64_t *src, const int64_t *dst, const uint8_t *label, double w_neg, double w_pos, const float *W,
                      double *loss_out, double *grad_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_lp_hess_workspace_bytes(int64_t n, int32_t d, int32_t models);
int ctgcn_lp_hess_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                      const int64_t *src, const int64_t *dst, const uint8_t *label, double w_neg, double w_pos, const float *W,
                      double *hess_out, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_lp_scores_f32(int64_t n, int32_t d, int32_t models, uint32_t measures, int64_t n_nodes, const float *E, int64_t lde,
                        const int64_t *src, const int64_t *dst, const float *W, float *score_out, void *stream);

/*
 * Centrality-prediction evaluation (evaluation/centrality_prediction.py; ctgcn_amd/evaluation/), ctgcn_cent.hip (ABI 31).
 * row_ptr / col: a symmetric int32 CSR without self loops, n vertices (n <= 2^31 - 1); all centralities are unweighted.
 *
 * ctgcn_cent_brandes: one BFS per source s in [s0, s1).  bc_out[v] (double[n]) = Σ_{s in range, s != v} δ_s(v), Brandes' dependency
 *   sums, UNSCALED (networkx's normalized undirected betweenness is bc · 1/((n-1)(n-2)) over all sources); r_out[s - s0] = vertices
 *   reached from s (s included), D_out[s - s0] = the sum of their distances (int64[s1 - s0]), the closeness counts.  Path counts and
 *   dependencies are fp64; sigma and delta are pulled over CSR rows in CSR order and per-block partials of bc are summed in a fixed
 *   order: repeated calls are bit-identical.  workspace: ctgcn_cent_brandes_workspace_bytes (a state slab per block, at most 2 GiB
 *   unless one slab is larger).
 * ctgcn_cent_eigenvector: networkx's eigenvector_centrality iteration: x = 1/n, then up to max_iter steps x <- (A+I)x / ||(A+I)x||_2
 *   (a zero norm counts as 1), stopping after the first step with Σ|x - x_last| < n·tol.  All steps are enqueued at once; after the
 *   stop test passes a device flag turns the rest into no-ops.  x_out (double[n]) holds x; *stop_step_host = the stop step
 *   (1-based), or 0 when no step passed the test.  One host read: the call synchronises `stream`.
 *   workspace: ctgcn_cent_eigenvector_workspace_bytes.
 * ctgcn_ridge_gram_{f32,f64}: the k-fold (KFold(folds), unshuffled: contiguous folds, the first n % folds one row longer) augmented
 *   Grams gram_out[f] = Zᵀ_f [X 1 Y]_f restricted to the rows of Z = [X 1] (double[folds, d+1, d+1+targets]), X row r at X + r*ldx,
 *   Y double[n, targets].  fp64 accumulation, per-chunk partials summed in a fixed order.  d <= 512 and targets <= 8, else
 *   CTGCN_E_UNSUPPORTED.  workspace: ctgcn_ridge_gram_workspace_bytes.
 * ctgcn_ridge_sse_{f32,f64}: sse_out[f, p] = Σ_{r in fold f} (Y[r, target_of[p]] - X[r]·W[f, p, :d] - W[f, p, d])² for models
 *   p < models <= 64, W double[folds, models, d+1], target_of int32[models] (device).  workspace: ctgcn_ridge_sse_workspace_bytes.
 */
size_t ctgcn_cent_brandes_workspace_bytes(int64_t n, int64_t s0, int64_t s1);
int ctgcn_cent_brandes(int64_t n, const int32_t *row_ptr, const int32_t *col, int64_t s0, int64_t s1, double *bc_out,
                       int64_t *r_out, int64_t *D_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_cent_eigenvector_workspace_bytes(int64_t n);
int ctgcn_cent_eigenvector(int64_t n, const int32_t *row_ptr, const int32_t *col, int32_t max_iter, double tol, double *x_out,
                           int32_t *stop_step_host, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_ridge_gram_workspace_bytes(int32_t d, int32_t targets, int32_t folds);
int ctgcn_ridge_gram_f32(int64_t n, int32_t d, int32_t targets, int32_t folds, const float *X, int64_t ldx, const double *Y,
                         double *gram_out, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_ridge_gram_f64(int64_t n, int32_t d, int32_t targets, int32_t folds, const double *X, int64_t ldx, const double *Y,
                         double *gram_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_ridge_sse_workspace_bytes(int32_t models, int32_t folds);
int ctgcn_ridge_sse_f32(int64_t n, int32_t d, int32_t targets, int32_t folds, int32_t models, const float *X, int64_t ldx,
                        const double *Y, const double *W, const int32_t *target_of, double *sse_out, void *workspace,
                        size_t workspace_bytes, void *stream);
int ctgcn_ridge_sse_f64(int64_t n, int32_t d, int32_t targets, int32_t folds, int32_t models, const double *X, int64_t ldx,
                        const double *Y, const double *W, const int32_t *target_of, double *sse_out, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * Node-classification evaluation (evaluation/node_classification.py; ctgcn_amd/evaluation/), ctgcn_nodecls.hip.
 * A launch covers `problems` independent one-vs-rest problems described by a problem table (all arrays on the device):
 *   - problem p owns the entries [row_start[p], row_start[p+1]) of rows (int64: a row of E, row v at E + v*lde, 1 <= d <= 256; rows
 *     outside [0, n_emb) read as zero) and y (int32: the entry's class index in [0, K_p));
 *   - problem p owns the models [model_start[p], model_start[p+1]) (int32).  The model arrays are indexed by m - model_start[0]:
 *     model_pos (int32: the positive class), model_w (double[models, 2]: balanced weights of the negative and positive rows),
 *     model_flag (int32: 0 fitted, 1 constant probability 0, 2 constant probability 1), the parameters W and the outputs;
 *   - chunk_start / part_start (int64[problems+1]): the blocks of problem p; the pass entry points need ctgcn_nc_chunks(n_p) blocks
 *     for a problem of n_p rows, the Hessian ctgcn_nc_hess_parts(n_p, hess_max).  total_chunks / total_parts = the last entry.
 *   - max_models >= the largest model count of a problem.  models = model_start[problems] - model_start[0].
 * Model m has z = w·x + b with (w, b) = W[m*(d+1) .. +d].  ctgcn_nc_grad_f32 and ctgcn_nc_predict_f32 take W as float[2, models, d+1]:
 * hi then lo parts (hi + lo = the fp64 parameters; lo may be zero); ctgcn_nc_hess_f32 takes float[models, d+1].  Each block gathers a
 * 32-row tile of its problem into LDS once for up to 64 models (32 when d > 131).  Per-block partials are summed per problem in block
 * order and the block count of a problem depends on its row count alone: a problem's outputs are bit-identical across calls and
 * whichever problems share the launch.
 *
 * ctgcn_nc_grad_f32: loss_out[m] = Σ_i s_i softplus(∓z_i) (double[models]) and grad_out[m*(d+1) + j] = Σ_i s_i (σ(z_i) - y_i) x̃_ij,
 *   x̃ = (x, 1) (double[models, d+1]), y_i = (y == model_pos[m]), s_i its balanced weight; zero for flagged models.  fp32 within a
 *   32-row tile, fp64 across tiles.  workspace: ctgcn_nc_grad_workspace_bytes.
 * ctgcn_nc_hess_f32: hess_out[m] = Σ_i s_i σ(1-σ) x̃_i x̃_iᵀ (double[models, d+1, d+1], symmetric) over the subsample i = 0, k, 2k, ...
 *   of each problem, k = ceil(n_p / hess_max) (every row when n_p <= hess_max), with the full set's weights; zero for flagged models.
 *   fp32 over parts of at most 1024 subsample rows, fp64 across parts.  workspace: ctgcn_nc_hess_workspace_bytes.
 * ctgcn_nc_predict_f32: problem p holds `groups` C groups of models, group-major: K_p = n_classes[p] models per group (classes
 *   0..K_p-1), or one model (class 1) when K_p = 2.  For every entry and group: pred_out[(entry - row_start[0])*groups + g] (int32) =
 *   the first argmax over the group's models of fp64 expit(z) (a flagged model contributes its constant; K_p = 2: class 1 iff
 *   p > 1 - p), and correct_out[p*groups + g] (int64) = the entries whose prediction equals y.  max_classes >= every K_p, at most
 *   64 (32 when d > 131), else CTGCN_E_UNSUPPORTED.
 *
 * Pair tables (edge classification, evaluation/edge_classification.py): ctgcn_ec_grad_f32 / ctgcn_ec_hess_f32 / ctgcn_ec_predict_f32
 * are the three entry points above with a second index array rows2 (int64, parallel to rows) directly after rows.  The feature of
 * entry i is then x_i = E[rows[i]] ⊙ E[rows2[i]]: one fp32 multiply per column, done while the tile is staged into LDS, so no
 * [entries, d] matrix is ever built; x_i is zero when either index lies outside [0, n_emb).  Everything else is the node table's:
 * the same kernels after the staging, the same return codes and argument checks (a null rows2 is CTGCN_E_INVALID), the same limit
 * d <= 256, and the same block counts and workspace sizes (ctgcn_nc_chunks, ctgcn_nc_hess_parts, ctgcn_nc_*_workspace_bytes), which
 * depend on a problem's row count alone; so a pair problem's outputs are bit-identical across calls and batch mates too, and equal
 * to those of a node table over the materialised fp32 products.  When d % 4 == 0, lde % 4 == 0 and E is 16-byte aligned the rows are
 * staged as float4 (half a wave per 512-byte row at d = 128, both endpoints of a wave's rows in flight together), else by the scalar
 * loop; both write the same values.
 */
int64_t ctgcn_nc_chunks(int64_t n);
int64_t ctgcn_nc_hess_parts(int64_t n, int64_t hess_max);
size_t ctgcn_nc_grad_workspace_bytes(int64_t total_chunks, int32_t d, int32_t max_models);
int ctgcn_nc_grad_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *chunk_start,
                      int64_t total_chunks, const int64_t *rows, const int32_t *y, const int32_t *model_start, const int32_t *model_pos,
                      const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E, int64_t lde, const float *W,
                      int64_t models, double *loss_out, double *grad_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_nc_hess_workspace_bytes(int64_t total_parts, int32_t d, int32_t max_models);
int ctgcn_nc_hess_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *part_start,
                      int64_t total_parts, int64_t hess_max, const int64_t *rows, const int32_t *y, const int32_t *model_start,
                      const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E,
                      int64_t lde, const float *W, int64_t models, double *hess_out, void *workspace, size_t workspace_bytes,
                      void *stream);
int ctgcn_nc_predict_f32(int32_t problems, int32_t d, int32_t max_classes, int32_t groups, const int64_t *row_start,
                         const int64_t *chunk_start, int64_t total_chunks, const int64_t *rows, const int32_t *y,
                         const int32_t *n_classes, const int32_t *model_start, const int32_t *model_flag, int64_t n_emb,
                         const float *E, int64_t lde, const float *W, int64_t models, int32_t *pred_out, int64_t *correct_out,
                         void *stream);
int ctgcn_ec_grad_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *chunk_start,
                      int64_t total_chunks, const int64_t *rows, const int64_t *rows2, const int32_t *y, const int32_t *model_start,
                      const int32_t *model_pos, const double *model_w, const int32_t *model_flag, int64_t n_emb, const float *E,
                      int64_t lde, const float *W, int64_t models, double *loss_out, double *grad_out, void *workspace,
                      size_t workspace_bytes, void *stream);
int ctgcn_ec_hess_f32(int32_t problems, int32_t d, int32_t max_models, const int64_t *row_start, const int64_t *part_start,
                      int64_t total_parts, int64_t hess_max, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                      const int32_t *model_start, const int32_t *model_pos, const double *model_w, const int32_t *model_flag,
                      int64_t n_emb, const float *E, int64_t lde, const float *W, int64_t models, double *hess_out, void *workspace,
                      size_t workspace_bytes, void *stream);
int ctgcn_ec_predict_f32(int32_t problems, int32_t d, int32_t max_classes, int32_t groups, const int64_t *row_start,
                         const int64_t *chunk_start, int64_t total_chunks, const int64_t *rows, const int64_t *rows2, const int32_t *y,
                         const int32_t *n_classes, const int32_t *model_start, const int32_t *model_flag, int64_t n_emb,
                         const float *E, int64_t lde, const float *W, int64_t models, int32_t *pred_out, int64_t *correct_out,
                         void *stream);

/*
 * Similarity-prediction evaluation (evaluation/similarity_prediction.py; ctgcn_amd/evaluation/), ctgcn_sim.hip.
 * The block: m vertices (the graph's non-isolated ones under a monotone relabel), row_ptr / col int32 and val double a symmetric
 * CSR with sorted columns, S double[m, m] row-major.
 *
 * ctgcn_sim_series: the columns [col0, col1) of S_iter_num, where S_1 = I and S_k = c·A·S_(k-1) + I (Leicht, Holme and Newman;
 *   the reference's dsd).  Every entry is the fp64 sum over its CSR row in CSR order, acc = acc + a_ij·x_j from +0.0, never fused,
 *   then c·acc + δ_ij: the reference's scipy product bit for bit.  The columns are walked in panels of `panel` (every step of a
 *   panel before the next one; one launch per step and panel); the result does not depend on `panel`.  iter_num >= 1.
 *   workspace: ctgcn_sim_series_workspace_bytes (two m x panel buffers).  ctgcn_sim_panel_cols: the default panel, the widest whose
 *   buffers and A stay inside the Infinity Cache.
 * ctgcn_sim_finish: in place, S <- (S + Sᵀ)/2 - I, then S <- (S - mn)/(mx - mn) with entries below eps set to 0, where mn, mx are
 *   the block's minimum and maximum, taken with 0 as well when pad_zero (the zero rows and columns of isolated vertices).
 *   stats_out (device double[2]) = mn, mx; row_nnz (device int64[m]) = the non-zeros left per row (NaN counts).
 *   workspace: ctgcn_sim_finish_workspace_bytes.
 * ctgcn_sim_coo: every non-zero of the finished S in row-major order: row i's at [row_off[i], row_off[i] + row_nnz[i]) of the
 *   outputs (row_off: device int64[m], the exclusive scan of row_nnz), as (ids[i], ids[j], S[i, j]), ids: device int64[m].
 * ctgcn_sim_gram_{f32,f64}: out (double[m, m]) = E_r E_rᵀ, E_r row a = E + rows[a]*lde (rows: device int64[m]), fp64 sums over
 *   k in order; each unordered pair is computed once and mirrored, so out is exactly symmetric.
 * ctgcn_sim_normalize: x (double[N]) <- (x - min)/(max - min), then x <- x / sum(x): the reference's two normalisations, with
 *   the sum formed in numpy's order (pairwise within chunks of 8192, chunks in order), so it is numpy's to the bit.
 *   stats_out (device double[3]) = min, max and the sum after the first step.  workspace: ctgcn_sim_normalize_workspace_bytes.
 * ctgcn_sim_spearman: xs / ys (double[N]) ascending with no NaN, xi / yi (int64[N]) their source positions (a torch.sort); every
 *   tie run gets its average rank, scattered back to the source positions, and sums_out (device double[3]) = Σ(rx-μ)(ry-μ),
 *   Σ(rx-μ)², Σ(ry-μ)² with μ = (N+1)/2.  workspace: ctgcn_sim_spearman_workspace_bytes.
 * All reductions are per-block partials summed in a fixed order with block counts set by the sizes: repeated calls are bit-identical.
 */
int64_t ctgcn_sim_panel_cols(int64_t m, int64_t nnz);
size_t ctgcn_sim_series_workspace_bytes(int64_t m, int64_t panel);
int ctgcn_sim_series(int64_t m, const int32_t *row_ptr, const int32_t *col, const double *val, double c, int32_t iter_num, int64_t panel,
                     int64_t col0, int64_t col1, double *S, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_sim_finish_workspace_bytes(int64_t m);
int ctgcn_sim_finish(int64_t m, int32_t pad_zero, double eps, double *S, double *stats_out, int64_t *row_nnz, void *workspace,
                     size_t workspace_bytes, void *stream);
int ctgcn_sim_coo(int64_t m, const double *S, const int64_t *row_off, const int64_t *ids, int32_t *row_out, int32_t *col_out,
                  double *data_out, void *stream);
int ctgcn_sim_gram_f32(int64_t m, int32_t d, const float *E, int64_t lde, const int64_t *rows, double *out, void *stream);
int ctgcn_sim_gram_f64(int64_t m, int32_t d, const double *E, int64_t lde, const int64_t *rows, double *out, void *stream);
size_t ctgcn_sim_normalize_workspace_bytes(int64_t N);
int ctgcn_sim_normalize(int64_t N, double *x, double *stats_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_sim_spearman_workspace_bytes(int64_t N);
int ctgcn_sim_spearman(int64_t N, const double *xs, const int64_t *xi, const double *ys, const int64_t *yi, double *sums_out,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Classifier head of the supervised trainer (reference models.py:46-125, metrics.py:169-209; ctgcn_amd/embedding.py), ctgcn_supervised.hip.
 * An item i is a labelled node a[i] (CTGCN_CLS_NODE, b unused) or a labelled pair (a[i], b[i]); its feature is f = E[a], f = E[a] ⊙ E[b]
 * (CTGCN_CLS_HADAMARD, one fp32 multiply per column, formed while a tile is staged: no [items, d] array exists) or, with no head behind
 * it, the score z = <E[a], E[b]> (CTGCN_CLS_DOT; W, bias, n_class and act are ignored).  a / b: device int64[items].  E: fp32 rows of
 * width d at stride lde (a [T, N, d] view of [N, T, d] is read in place).  W: fp32 [n_class, d] row-major, bias: [n_class] or null.
 * Limits: 1 <= d <= 256 and 2 <= n_class <= 32, else CTGCN_E_UNSUPPORTED.
 *
 * ctgcn_cls_check_items: the host check of the index arrays: copies them to the host (synchronises `stream`, launches nothing) and
 *   returns CTGCN_E_INVALID when an index lies outside [0, n_nodes).  Index sets do not change between epochs, so a caller checks a set
 *   once; the kernels themselves give an item with an index out of range a zero feature and never read or write outside E / dE.
 * ctgcn_cls_head_fwd_f32: out[i, c] = act(W[c]·f_i + bias[c]), act 0 the identity ('L'), 1 SELU ('N'); DOT: out[i] = z_i.
 * ctgcn_cls_loss_f32: over logits [items, n_class] and labels int64 in [0, n_class): mean cross entropy to loss_out (device double[1]),
 *   the number of rows whose first maximal class is the label to correct_out (device int64[1]), softmax to prob and
 *   dlogits = (p - onehot) / items, times SELU'(.) from the activated logits when act is 1 (so dlogits is the gradient at the Linear's
 *   output).  DOT: logits [items], labels in {0, 1}, BCE with logits, z > 0 predicts 1, prob = σ(z), dlogits = (σ(z) - y) / items.
 *   prob and dlogits may be null.  workspace: ctgcn_cls_loss_workspace_bytes.
 * ctgcn_cls_head_bwd_f32: from dlogits, dE (rows at stride ldde; null: skipped) in pull form and dW [n_class, d] / db [n_class] (null:
 *   skipped; DOT has neither).  The caller supplies the incidence lists of the item set, built once per set:
 *     inc_item / inc_other int64[incidences]: per node, in a fixed order, the items it takes part in and the other endpoint of each
 *       (NODE: one incidence per item, inc_other unused; pairs: two per item, a pair with a == b twice in its node's list);
 *     pieces: every node's list cut into ceil(len / ctgcn_cls_pull_piece()) pieces, at least one (an empty one for a node with no
 *       item, whose dE row is written as zeros), in node order: piece p is [piece_ptr[p], piece_ptr[p+1]) of node piece_node[p];
 *     piece_slot[p]: -1 when the node has one piece (the row goes to dE), else the piece's row in the fp64 partial buffer;
 *     hubs: the nodes with several pieces, hub_node int64[n_hubs]; their partial rows are [hub_slot_ptr[h], hub_slot_ptr[h+1]),
 *       hub_pieces in all, added in piece order.
 *   NODE: dE[v] = Wᵀ Σ dlogits_i; HADAMARD: Σ (Wᵀ dlogits_i) ⊙ E[other]; DOT: Σ dlogits_i E[other]; sums in list order.
 *   workspace: ctgcn_cls_head_bwd_workspace_bytes(items, d, n_class (1 for DOT), hub_pieces).
 * No float atomics; block and piece counts depend on the sizes alone, sums run in fp64 in a fixed order: repeated calls are bit-identical.
 */
#define CTGCN_CLS_NODE 0
#define CTGCN_CLS_HADAMARD 1
#define CTGCN_CLS_DOT 2
int64_t ctgcn_cls_pull_piece(void);
int ctgcn_cls_check_items(int32_t mode, int64_t items, const int64_t *a, const int64_t *b, int64_t n_nodes, void *stream);
int ctgcn_cls_head_fwd_f32(int32_t mode, int32_t act, int64_t items, int32_t d, int32_t n_class, const int64_t *a, const int64_t *b,
                           int64_t n_nodes, const float *E, int64_t lde, const float *W, const float *bias, float *out, void *stream);
size_t ctgcn_cls_loss_workspace_bytes(int64_t items);
int ctgcn_cls_loss_f32(int32_t mode, int32_t act, int64_t items, int32_t n_class, const float *logits, const int64_t *labels,
                       double *loss_out, int64_t *correct_out, float *prob, float *dlogits, void *workspace, size_t workspace_bytes,
                       void *stream);
size_t ctgcn_cls_head_bwd_workspace_bytes(int64_t items, int32_t d, int32_t n_class, int64_t hub_pieces);
int ctgcn_cls_head_bwd_f32(int32_t mode, int64_t items, int32_t d, int32_t n_class, const int64_t *a, const int64_t *b, int64_t n_nodes,
                           const float *E, int64_t lde, const float *W, const float *dlogits, int64_t n_pieces, const int64_t *piece_ptr,
                           const int64_t *piece_node, const int64_t *piece_slot, const int64_t *inc_item, const int64_t *inc_other,
                           int64_t n_hubs, const int64_t *hub_node, const int64_t *hub_slot_ptr, int64_t hub_pieces, float *dE,
                           int64_t ldde, float *dW, float *db, void *workspace, size_t workspace_bytes, void *stream);

/*
 * GCN step of the EvolveGCN baseline (reference baseline/egcn.py:74, helper.py:27-47; ctgcn_amd/baseline/egcn.py), ctgcn_gcn.hip.
 * The matrix is an int32 CSR with fp32 values, n < 2^31 rows; the layer kernels take it as given (already normalised).
 *
 * ctgcn_gcn_normalize_f32: over a CSR that already holds the diagonal, val_out[e] = float(r_i · val_in[e] · (row_norm ? 1 : r_j)) with
 *   r_i = rowsum_i^-1 (row_norm 1) or rowsum_i^-1/2 (row_norm 0), row sums, r and the product in fp64, one rounding to fp32; r_i = 0 for
 *   a zero row sum.  *flag (device int32) is cleared by the call and set to 1 when a row sum is negative (the caller reads it and
 *   raises).  workspace: ctgcn_gcn_normalize_workspace_bytes(n) bytes (the n scales), 8-byte aligned.
 * ctgcn_gcn_layer_fwd_f32: Y[i] = act(Σ_e val[e] · S[col[e]]); act 0 the identity, 1 F.rrelu in eval mode (y >= 0 ? y : y · 11/48).
 *   score_vec [d] and score_out [n], both or neither: score_out[i] = Y[i] · score_vec.
 * ctgcn_gcn_layer_bwd_f32: dS[i] = Σ_e val[e] · (dY[col[e]] ∘ m(Y[col[e]])) over the SAME CSR (the caller guarantees a symmetric matrix);
 *   m = 1 for act 0 (Y may be null), for act 1 m(y) = y > 0 ? 1 : 11/48, formed on the gathered row.
 * Rows at strides lds / ldy / lddy / ldds >= d; float4 accesses when d, the strides and the pointers allow, else scalar.
 * long_rows int32[n_long] must list exactly the rows with more than long_threshold entries (null / 0: every row is handled by its lane
 *   group).  A long row is cut into ceil(len / (4 · long_threshold)) pieces, at most as many as the workspace holds:
 *   workspace_bytes >= n_long · pieces · round_up(d, 4) · 4, 16-byte aligned, at least one piece per row (else CTGCN_E_WORKSPACE); with
 *   fewer pieces than a row asks for its pieces grow.  n_long <= 65535.
 * No atomics; every sum has a fixed order: repeated calls on the same inputs are bit-identical.
 */
size_t ctgcn_gcn_normalize_workspace_bytes(int64_t n);
int ctgcn_gcn_normalize_f32(int64_t n, const int32_t *row_ptr, const int32_t *col, const float *val_in, int32_t row_norm, float *val_out,
                            int32_t *flag, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_gcn_layer_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S, int64_t lds,
                            float *Y, int64_t ldy, int32_t act, const float *score_vec, float *score_out, const int32_t *long_rows,
                            int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_gcn_layer_bwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *dY,
                            int64_t lddy, const float *Y, int64_t ldy, int32_t act, float *dS, int64_t ldds, const int32_t *long_rows,
                            int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);

/*
 * GCN step of the GCN / GCRN baselines (reference baseline/gcn.py:36-43, :84-88, baseline/gcrn.py:56-57; ctgcn_amd/baseline/gcn.py,
 * gcrn.py), ctgcn_gcn.hip.  Same CSR, long-row and workspace rules as ctgcn_gcn_layer_fwd_f32; the matrix need not be symmetric.
 *
 * ctgcn_gcn_conv_fwd_f32: Y[i] = epi(Σ_e val[e] · S[col[e]] + bias); bias [d] may be null.  epi:
 *   0  none;
 *   1  ReLU, then dropout when p > 0: entry (i, c) is kept iff u01(key, i, c) >= p (ctgcn_rng.h's splitmix64 draw, compared in
 *      double) and scaled by 1 / (1 - p) in fp32; zero where dropped or where the sum is <= 0.  p = 0 is bit-identical to plain ReLU;
 *   2  the row's L2 normalisation Y[i] = x / max(‖x‖₂, 1e-12) (F.normalize), with norm[i] = ‖x‖₂ written as well (norm required).
 *   0 <= p < 1 is checked for every epi and used by epi 1 only.
 * ctgcn_gcn_conv_prep_f32: the backward's N x d pass.  G = d loss / d (the sum before the epilogue) from dY and the forward's Y:
 *   1  G = Y > 0 ? dY / (1 - p) : 0 (an entry was kept and positive exactly when Y > 0: no mask, no key);
 *   2  G = (dY − Y ⟨Y, dY⟩) / norm where norm >= 1e-12, else dY / 1e-12 (the clamped denominator is a constant);
 *   0  G = dY: nothing is written, Y / G / norm may be null.
 *   db [d], when not null, receives Σ_i G[i]: per-block partial sums in the workspace (ctgcn_gcn_conv_prep_workspace_bytes(n, d) bytes,
 *   16-byte aligned; ctgcn_gcn_conv_prep_rows() rows per block), added in block order by a second launch.
 * The input gradient is then dS = Âᵀ G: ctgcn_gcn_conv_fwd_f32 with epi 0 and no bias over the transposed CSR.
 * No atomics; every sum has a fixed order: repeated calls on the same inputs are bit-identical.
 */
int ctgcn_gcn_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S, int64_t lds,
                           const float *bias, float *Y, int64_t ldy, int32_t epi, double p, uint64_t key, float *norm,
                           const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                           void *stream);
int32_t ctgcn_gcn_conv_prep_rows(void);
size_t ctgcn_gcn_conv_prep_workspace_bytes(int64_t n, int32_t d);
int ctgcn_gcn_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *norm, int32_t epi,
                            double p, float *G, int64_t ldg, float *db, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Graph-attention step of the GAT baseline (reference baseline/gat.py:65-105; ctgcn_amd/baseline/gat.py), ctgcn_gat.hip.
 * One layer: `heads` heads of width F = d / heads over S [n, d] (columns [hF, (h+1)F) hold x W_h), a_src / a_dst [heads, F], and the
 * pattern of a CSR (row_ptr / col and the long-row list as in ctgcn_gcn_layer_fwd_f32; the values are not read).  For entry (i, j):
 *   z = u_i + v_j, l = -leakyrelu_alpha(z), m_i = max_j l, e = exp(l - m_i), Z_i = Σ_j e, q = keep(key + h, i, j) / (1 - p_att),
 *   Y_i^h = (Σ_j q e S_j^h) / Z_i;  keep(k, i, j) = u01(k, i, j) >= p_att (ctgcn_rng.h, compared in double); p_att = 0 draws nothing.
 *   A row without entries gives exact zeros (and m = Z = 0).
 * ctgcn_gat_fwd_f32: u, v, m, Z [n, heads] and out = epi(Y) are written.  epi: 0 none; 1 ELU; 2 ELU, then feature dropout when
 *   p_feat > 0: entry (i, c) kept iff u01(fkey, i, c) >= p_feat, scaled by 1 / (1 - p_feat).  With epi != 0, Y [n, d] receives the sums
 *   before the epilogue, which the backward reads (Y may be null with epi 0: out is Y).
 * ctgcn_gat_bwd_prep_f32: G = d loss / d Y from dY through the epilogue (mask regenerated from fkey; with epi 0 nothing is written
 *   and G = dY), D_i = G_i^h · Y_i^h, and pack [n, heads, 4] = {u, m, 1 / Z (0 where Z = 0), D}, 16-byte aligned.
 * ctgcn_gat_bwd_row_f32: over the CSR.  R_i^h = Σ_j s q p S_j^h (p = e / Z_i, s = z > 0 ? 1 : alpha), csum_i = Σ_j s p, then
 *   du_i = D_i csum_i − G_i^h · R_i^h.  R [n, d] and csum [n, heads] are scratch of the call.
 * ctgcn_gat_bwd_col_f32: over the transposed CSR (row_ptr / col / long rows of Aᵀ).  A_j^h = Σ_i q p G_i^h into dS, B_j^h = Σ_i s q p G_i^h,
 *   ksum_j = Σ_i s p D_i, then dv_j = ksum_j − S_j^h · B_j^h and dS_j^h = A_j^h + du_j a_src_h + dv_j a_dst_h.  B [n, d] and ksum
 *   [n, heads] are scratch.  du and dS may both be null: dv alone.
 * ctgcn_gat_da_f32: da_src [heads, F] = Σ_i du_i S_i^h and da_dst = Σ_i dv_i S_i^h from one read of S: per-block column sums in the
 *   workspace (ctgcn_gat_da_workspace_bytes(n, d) bytes), added in block order by a second launch.  du / da_src or dv / da_dst may
 *   be null together; n = 0 writes zeros.
 * Long rows: workspace of n_long · pieces · ctgcn_gat_piece_floats(d, heads) · 4 bytes, 16-byte aligned (at least one piece per row).
 * Returns CTGCN_E_INVALID for null pointers, n < 0 or n >= 2^31, d < 1, heads < 1, d % heads != 0, a leading dimension below d, a p
 * outside [0, 1) or a non-finite alpha; CTGCN_E_WORKSPACE for a workspace that is too small; 0 for n = 0.
 * No atomics; every sum has a fixed order: repeated calls on the same inputs are bit-identical.
 */
int32_t ctgcn_gat_piece_floats(int32_t d, int32_t heads);
size_t ctgcn_gat_da_workspace_bytes(int64_t n, int32_t d);
int ctgcn_gat_da_f32(int64_t n, int32_t d, int32_t heads, const float *S, int64_t lds, const float *du, const float *dv, float *da_src,
                     float *da_dst, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_gat_fwd_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                      const float *a_src, const float *a_dst, double alpha, int32_t epi, double p_att, uint64_t key, double p_feat,
                      uint64_t fkey, float *out, int64_t ldout, float *Y, int64_t ldy, float *u, float *v, float *m, float *Z,
                      const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                      void *stream);
int ctgcn_gat_bwd_prep_f32(int64_t n, int32_t d, int32_t heads, const float *dY, int64_t lddy, const float *Y, int64_t ldy, int32_t epi,
                           double p_feat, uint64_t fkey, const float *u, const float *m, const float *Z, float *G, int64_t ldg, void *pack,
                           void *stream);
int ctgcn_gat_bwd_row_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                          const float *G, int64_t ldg, const float *v, const void *pack, double alpha, double p_att, uint64_t key, float *R,
                          int64_t ldr, float *csum, float *du, const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                          void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_gat_bwd_col_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *G, int64_t ldg,
                          const float *S, int64_t lds, const float *v, const void *pack, const float *a_src, const float *a_dst, double alpha,
                          double p_att, uint64_t key, const float *du, float *dS, int64_t ldds, float *B, int64_t ldb, float *ksum, float *dv,
                          const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                          void *stream);

/*
 * PyTorch-Geometric variants of the GCN, GAT, GraphSAGE and GIN baselines (reference TgGCN, TgGAT, TgSAGE, TgGIN;
 * ctgcn_amd/baseline/tg.py), ctgcn_tg.hip and the PyG-form entry points of ctgcn_gat.hip.
 *
 * The operator of a raw edge index (src / dst int64 [E], node ids in [0, n); row = target, stored columns = sources):
 * ctgcn_tg_keys: keys[e] = dst[e] · n + src[e]; an index outside [0, n) gives the key n · n and sets *flag (int32, zeroed by the caller).
 * ctgcn_tg_csr_count: over the keys sorted ascending.  raw_ptr [n + 1]: row pointers of the pairs as given; loop_at [n]: the entries
 *   of row v whose source is below v; nloops [n]: the loops (v, v) the input holds.  Binary searches, no atomics.
 * ctgcn_tg_csr_emit: col [E] = the sources in key order, mean [E] = 1 / (entries of the row).  The looped pattern of GCNConv and
 *   GATConv over looped_ptr [n + 1] (row length c_v = raw length − nloops[v] + 1, scanned by the caller): every non-loop entry at its
 *   sorted position, a repeated pair as a repeated entry, exactly one loop per node; val_l = dis_s · dis_t with dis_v = c_v^-1/2,
 *   formed in fp64 and rounded once.  col_l / val_l hold looped_ptr[n] <= E + n entries.
 * Need 0 <= n < 2^31 and 0 <= E < 2^31 − n (CTGCN_E_INVALID otherwise).
 *
 * ctgcn_tg_conv_fwd_f32: Y[i] = epi(Σ_e val[e] · S[col[e]] + self_scale · T[i] + bias) over a CSR with the long-row rules of
 *   ctgcn_gcn_conv_fwd_f32.  T and bias may be null; T may be S or another column slice of S's buffer.  epi 0 none; 1 ReLU, then
 *   dropout when p > 0: entry (i, c) kept iff u01(key, i, c) >= p and scaled by 1 / (1 − p).
 * ctgcn_tg_conv_prep_f32: the backward's N x d pass.  With epi 1, G = dY where Y + bias > 0 (bias null: Y alone, the saved output)
 *   and the draw, made again from key, kept the entry (scaled by 1 / (1 − p)), else 0; with epi 0 nothing is written and G = dY.
 *   db [d], when not null, receives Σ_i G[i]: per-block partial sums in the workspace (ctgcn_tg_prep_workspace_bytes(n, d) bytes,
 *   16-byte aligned), added in block order by a second launch.  epi 0 without db is refused: there is nothing to compute.
 *
 * ctgcn_tgat_fwd_f32, ctgcn_tgat_bwd_row_f32, ctgcn_tgat_bwd_col_f32: ctgcn_gat_*'s passes in GATConv's form.  a_tgt pairs with the
 *   row's own features (u_i = a_tgt_h · S_i^h), a_src with the gathered ones (v_j = a_src_h · S_j^h); l = +leakyrelu_slope(u_i + v_j),
 *   m_i = max_j l, Y_i^h = (Σ_j e S_j^h) / Z_i, out = epi(Y + bias) with epi and the dropout of ctgcn_tg_conv_fwd_f32; no attention
 *   dropout.  Y [n, d] receives the sums before the bias whenever bias is not null or epi is 1 (else out is Y and Y may be null); an
 *   empty row gives Y = 0, out = epi(bias).  The backward takes G from ctgcn_tg_conv_prep_f32 (Y, bias) and pack from
 *   ctgcn_gat_bwd_prep_f32 with epi 0 on that G; du_i = G_i^h · R_i^h − D_i csum_i and dv_j = S_j^h · B_j^h − ksum_j (dl / dz = s
 *   where the reference form has −s); ctgcn_gat_da_f32 is shared.  The row pass sums with s − s0_i in place of s, s0_i the slope at
 *   the row's largest logit: Σ_j p (t − D_i) = 0, so du is unchanged, and exactly 0 for a row whose logits share a sign.  It also
 *   takes Y (the forward's sums before the bias) and gathers S_j − Y_i: t − D_i = G_i · (S_j − Y_i), so du_i = G_i^h · R_i^h with csum
 *   left at 0, and a component all S_j share never enters the sum.
 * Argument checks, long rows, float4 rule and determinism as for the entry points they stand beside.
 */
int ctgcn_tg_keys(int64_t E, int64_t n, const int64_t *src, const int64_t *dst, int64_t *keys, int32_t *flag, void *stream);
int ctgcn_tg_csr_count(int64_t E, int64_t n, const int64_t *keys, int32_t *raw_ptr, int32_t *loop_at, int32_t *nloops, void *stream);
int ctgcn_tg_csr_emit(int64_t E, int64_t n, const int64_t *keys, const int32_t *raw_ptr, const int32_t *loop_at, const int32_t *nloops,
                      const int32_t *looped_ptr, int32_t *col, float *mean, int32_t *col_l, float *val_l, void *stream);
int ctgcn_tg_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S, int64_t lds,
                          const float *T, int64_t ldt, float self_scale, const float *bias, float *Y, int64_t ldy, int32_t epi, double p,
                          uint64_t key, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                          size_t workspace_bytes, void *stream);
size_t ctgcn_tg_prep_workspace_bytes(int64_t n, int32_t d);
int ctgcn_tg_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *bias, int32_t epi,
                           double p, uint64_t key, float *G, int64_t ldg, float *db, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_tgat_fwd_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                       const float *a_tgt, const float *a_src, double slope, const float *bias, int32_t epi, double p, uint64_t key,
                       float *out, int64_t ldout, float *Y, int64_t ldy, float *u, float *v, float *m, float *Z, const int32_t *long_rows,
                       int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_tgat_bwd_row_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds,
                           const float *G, int64_t ldg, const float *Y, int64_t ldy, const float *v, const void *pack, double slope, float *R,
                           int64_t ldr, float *csum, float *du, const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                           void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_tgat_bwd_col_f32(int64_t n, int32_t d, int32_t heads, const int32_t *row_ptr, const int32_t *col, const float *G, int64_t ldg,
                           const float *S, int64_t lds, const float *v, const void *pack, const float *a_tgt, const float *a_src, double slope,
                           const float *du, float *dS, int64_t ldds, float *B, int64_t ldb, float *ksum, float *dv, const int32_t *long_rows,
                           int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Pooling layers of the GIN and GraphSAGE baselines (reference baseline/gin.py, baseline/sage.py; ctgcn_amd/baseline/gin.py, sage.py),
 * ctgcn_pool.hip.  Same CSR and long-row rules as ctgcn_gcn_conv_fwd_f32; the matrix need not be symmetric.
 *
 * ctgcn_pool_conv_fwd_f32: Y[i] = epi(Σ_e val[e] · S[col[e]] + self_scale · T[i] + bias).  T [n, d] (row stride ldt) and bias [d] may
 *   be null; T may be S itself or another column slice of S's buffer.  row_ptr null: no matrix (every row empty; col, val, S unused).
 *   epi 0 none; 1 ReLU, then the row's L2 normalisation x / max(‖x‖₂, 1e-12) with norm[i] = ‖x‖₂ (norm required), then dropout when
 *   p > 0: entry (i, c) kept iff u01(key, i, c) >= p and scaled by 1 / (1 - p).  With p > 0 Ysave [n, d], when not null, receives the
 *   normalised rows before dropout, which the backward reads (with p = 0 that is Y).
 * ctgcn_pool_conv_prep_f32: the backward's N x d pass of epi 1.  g = dY through the dropout draw (made again from key), then
 *   G = Y > 0 ? (g − Y ⟨Y, g⟩) / norm : 0 where norm >= 1e-12, else Y > 0 ? g / 1e-12 : 0; Y the normalised rows before dropout.
 *   db [d], when not null, receives Σ_i G[i]: per-block partial sums in the workspace (ctgcn_pool_prep_workspace_bytes(n, d) bytes,
 *   16-byte aligned), added in block order by a second launch.  Then dT = self_scale · G and dS = Âᵀ G (ctgcn_gcn_conv_fwd_f32 over
 *   the transposed CSR).
 * ctgcn_pool_max_fwd_f32: Y[i, c] = max_e S[col[e], c] and arg[i, c] = the col[e] that holds it, the lowest among equal values; an
 *   empty row gives 0 and -1.  The values of the matrix are not read.  Long rows: workspace of n_long · pieces · round_up(d, 4) · 8
 *   bytes (the partial maxima and their indices).
 * ctgcn_pool_max_bwd_f32: over the transposed CSR (row_ptr / col / long rows of Aᵀ): dS[j, c] = Σ_{i in row j of Aᵀ} [arg[i, c] == j] ·
 *   dY[i, c], in the stored (ascending) order of i.  Long rows: workspace of n_long · pieces · round_up(d, 4) · 4 bytes.
 * ctgcn_bn_stats_f32: per-column mean, biased variance and rstd = 1 / sqrt(var + eps) over the n >= 1 rows of x.  Blocks of
 *   ctgcn_bn_stats_rows() rows sum x − K and (x − K)² in fp64 (K the block's first row) into a (mean, M2) pair per block and column
 *   in the workspace (ctgcn_bn_stats_workspace_bytes(n, d) bytes, 8-byte aligned); a second launch merges the pairs by Chan's
 *   formula in fp64 in a fixed order.
 * ctgcn_bn_apply_f32: y = dropout(relu((x − mean) · rstd · weight + bias)); relu 0 or 1, dropout as above when p > 0.
 * ctgcn_bn_bwd_f32: g = dy through the dropout draw and the ReLU mask, both made again from x; db = Σ_i g, dw = Σ_i g ⊙ x̂ as per-block
 *   column sums added in block order (workspace of ctgcn_bn_bwd_workspace_bytes(n, d) bytes, 16-byte aligned); then, when dx is not
 *   null, dx = weight · rstd · (g − db / n − x̂ · dw / n) with batch_stats 1, weight · rstd · g with 0 (statistics given, eval mode).
 * float4 rows when d, every leading dimension and every base address allow it, scalar rows otherwise.
 * Returns CTGCN_E_INVALID for null pointers, n < 0 or n >= 2^31, d < 1, a leading dimension below d or a p outside [0, 1);
 * CTGCN_E_WORKSPACE for a workspace that is too small; 0 for n = 0 (ctgcn_bn_stats_f32 needs n >= 1).
 * CTGCN_E_UNSUPPORTED for more than 65535 long rows in the three gather entries (raise long_threshold), for more than 65535 statistics
 * blocks in ctgcn_bn_stats_f32 (n above 65535 · ctgcn_bn_stats_rows() = 8 388 480 rows), and for n · d beyond a grid of 2^31 − 1 blocks
 * of 256 in the apply and backward passes.
 * No atomics; every sum has a fixed order: repeated calls on the same inputs are bit-identical.
 */
int ctgcn_pool_conv_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S, int64_t lds,
                            const float *T, int64_t ldt, float self_scale, const float *bias, float *Y, int64_t ldy, int32_t epi, double p,
                            uint64_t key, float *norm, float *Ysave, int64_t ldsave, const int32_t *long_rows, int32_t n_long,
                            int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_pool_prep_workspace_bytes(int64_t n, int32_t d);
int ctgcn_pool_conv_prep_f32(int64_t n, int32_t d, const float *dY, int64_t lddy, const float *Y, int64_t ldy, const float *norm, double p,
                             uint64_t key, float *G, int64_t ldg, float *db, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_pool_max_fwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *S, int64_t lds, float *Y,
                           int64_t ldy, int32_t *arg, int64_t ldarg, const int32_t *long_rows, int32_t n_long, int32_t long_threshold,
                           void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_pool_max_bwd_f32(int64_t n, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *dY, int64_t lddy,
                           const int32_t *arg, int64_t ldarg, float *dS, int64_t ldds, const int32_t *long_rows, int32_t n_long,
                           int32_t long_threshold, void *workspace, size_t workspace_bytes, void *stream);
int32_t ctgcn_bn_stats_rows(void);
size_t ctgcn_bn_stats_workspace_bytes(int64_t n, int32_t d);
int ctgcn_bn_stats_f32(int64_t n, int32_t d, const float *x, int64_t ldx, double eps, float *mean, float *var, float *rstd, void *workspace,
                       size_t workspace_bytes, void *stream);
int ctgcn_bn_apply_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *mean, const float *rstd, const float *weight,
                       const float *bias, int32_t relu, double p, uint64_t key, float *y, int64_t ldy, void *stream);
size_t ctgcn_bn_bwd_workspace_bytes(int64_t n, int32_t d);
int ctgcn_bn_bwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *dy, int64_t lddy, const float *mean, const float *rstd,
                     const float *weight, const float *bias, int32_t relu, double p, uint64_t key, int32_t batch_stats, float *dx,
                     int64_t lddx, float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The P-GNN baseline (reference baseline/pgnn.py; ctgcn_amd/baseline/pgnn.py), ctgcn_pgnn.hip.
 *
 * ctgcn_pgnn_anchor_dist: for n_sets anchor sets, packed as offsets [n_sets + 1] (ascending from 0 to n_members) and members
 *   [n_members] (node ids, a set may list a node twice), a multi-source BFS per set over the pattern of the CSR (values are not read;
 *   self-loops, repeated entries and column indices outside [0, n) are harmless; the pattern is taken as given, so an undirected graph
 *   is a symmetric pattern).  cutoff <= 0: exact; > 0: nodes within that many hops.  Outputs, each [n, n_sets] with the set index
 *   fastest: level (hops to the closest anchor of the set, -1 unreached; int32, so no distance wraps), dist_max = 1 / (level + 1) as
 *   fp32 division (0 unreached), pos = the position inside the set of the closest anchor, the smallest among equally close ones (0
 *   unreached): the reference's np.max / np.argmax over its dense matrix; node_id, when not null, members[offsets[s] + pos] (0 for an
 *   empty set).  levels_run_host (may be null) receives the number of passes.  The only atomic is an integer minimum while seeding;
 *   results do not depend on the order of execution.  workspace: ctgcn_pgnn_dist_workspace_bytes() bytes.  Reads a flag back after every pass:
 *   synchronises `stream`.  CTGCN_E_INVALID for bad sizes, null pointers, offsets that do not ascend from 0 to n_members or a member
 *   outside [0, n); CTGCN_E_UNSUPPORTED when n · n_sets reaches 2^31.
 *
 * ctgcn_pgnn_conv_fwd_f32: PS [n, 2 d] = P | S (row stride ldps), lvl and idx int32 [n, n_sets] (entries are clamped into
 *   [0, n_table) and [0, n)), table [n_table], w_p [d], b_p [1] or null.  m = relu(table[lvl[i, a]] · P[idx[i, a]] + S[i]);
 *   pos[i, a] = ⟨m, w_p⟩ + b_p and strct[i] = mean_a m; each is computed when its pointer is not null, at least one.  normalize 1:
 *   pos rows are divided by max(‖row‖₂, 1e-12) and xraw [n, n_sets] receives pos before that, which the backward reads.  p > 0: entry (i, c) of strct is kept iff
 *   u01(key, i, c) >= p and scaled by 1 / (1 − p).  1 <= d <= 512, n_sets >= 1.
 * ctgcn_pgnn_conv_bwd_row_f32: per node, with everything per (i, a, c) made again, gm = (gx[i, a] · w_p + gs[i] / n_sets) ⊙ [m > 0]
 *   where gx is g_pos taken back through the normalisation (in fp64, from xraw) when normalize, and gs is
 *   g_struct through the dropout draw made again; g_pos or g_struct may be null (that output was not asked for).  Writes
 *   gPS[i, d:] = Σ_a gm, gd[i, a] = ⟨gm, P[idx]⟩, gx [n, n_sets] when normalize, gse [n, d] = gs / n_sets when g_struct is given, and
 *   g_w [d] = Σ m · gx, g_b [1] = Σ gx as per-block partial sums (ctgcn_pgnn_bwd_row_workspace_bytes(n, d) bytes) added in block order.
 * ctgcn_pgnn_conv_bwd_pull_f32: gPS[j, :d] = Σ_{(i, a): idx = j} d' · gm over the transposed index: perm [n · n_sets] the items
 *   i · n_sets + a sorted by idx (ascending inside a node's list), pieces int32 [4][n_pieces] = node, lo, hi (a range of perm) and dst
 *   (>= 0: the piece is the node's whole list and is written to that row of gPS; < 0: to row −1 − dst of the workspace; a row at or beyond part_rows is not written), multi_node
 *   [n_multi] / multi_ptr [n_multi + 1]: the nodes with several pieces and their workspace rows, added in order.  gx is g_pos itself
 *   without normalisation, or null; gse as written by the row pass, or null.  Rows of gPS[:, :d] of nodes nobody chose are not
 *   written.  workspace: ctgcn_pgnn_bwd_pull_workspace_bytes(part_rows, d).
 * ctgcn_pgnn_table_grad_f32: g_table[u] = Σ_{lvl = u} gd over perm (the items sorted by lvl), pieces int32 [2][n_pieces] = lo, hi,
 *   piece_ptr [n_table + 1] the pieces of each entry; a block sums a piece in a fixed order, the pieces are added in order.
 * Returns CTGCN_E_INVALID for null pointers and bad sizes, CTGCN_E_UNSUPPORTED for d > 512 or n · n_sets >= 2^31,
 * CTGCN_E_WORKSPACE for a workspace that is too small; 0 for n = 0.  No float atomics; repeated calls are bit-identical.
 * The sums over anchor sets, nodes, list items and blocks are kept in fp64; what is written is fp32.
 */
size_t ctgcn_pgnn_dist_workspace_bytes(void);
int ctgcn_pgnn_anchor_dist(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, int32_t n_sets, const int32_t *offsets,
                           const int32_t *members, int32_t n_members, int32_t cutoff, int32_t *level, float *dist_max, int32_t *pos,
                           int32_t *node_id, int32_t *levels_run_host, void *workspace, size_t workspace_bytes, void *stream);
int ctgcn_pgnn_conv_fwd_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl, const float *table,
                            int32_t n_table, const int32_t *idx, const float *w_p, const float *b_p, float *pos, float *strct,
                            int64_t ldstruct, int32_t normalize, float *xraw, double p, uint64_t key, void *stream);
size_t ctgcn_pgnn_bwd_row_workspace_bytes(int64_t n, int32_t d);
int ctgcn_pgnn_conv_bwd_row_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl, const float *table,
                                int32_t n_table, const int32_t *idx, const float *w_p, const float *g_pos, const float *xraw,
                                int32_t normalize, const float *g_struct, int64_t ldgs, double p, uint64_t key,
                                float *gPS, int64_t ldg, float *gd, float *gx, float *gse, int64_t ldgse, float *g_w, float *g_b,
                                void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_pgnn_bwd_pull_workspace_bytes(int64_t part_rows, int32_t d);
int ctgcn_pgnn_conv_bwd_pull_f32(int64_t n, int32_t n_sets, int32_t d, const float *PS, int64_t ldps, const int32_t *lvl, const float *table,
                                 int32_t n_table, const float *w_p, const float *gx, const float *gse, int64_t ldgse, const int32_t *perm,
                                 const int32_t *pieces, int64_t n_pieces, const int32_t *multi_node, const int32_t *multi_ptr,
                                 int64_t n_multi, int64_t part_rows, float *gPS, int64_t ldg, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t ctgcn_pgnn_table_grad_workspace_bytes(int64_t n_pieces);
int ctgcn_pgnn_table_grad_f32(int64_t items, int32_t n_table, const float *gd, const int32_t *perm, const int32_t *pieces, int64_t n_pieces,
                              const int32_t *piece_ptr, float *g_table, void *workspace, size_t workspace_bytes, void *stream);

/* ---- decoder loss of the VGRNN baseline (ctgcn_vgrnn.hip): reference baseline/vgrnn.py:402-413 and metrics.py:154-161 without a dense
 * [n, n] matrix.  With S the sum of the stored adjacency values, posw = (n² − S) / S and x_ij = z_i · z_j,
 *   nll = [ Σ_ij softplus(x_ij) + Σ_stored a_e ((posw − 1) softplus(−x_e) − x_e) ] / (2 (n² − S)).
 * ctgcn_vae_nll_dense_f32: loss[0] (fp64, device) = Σ_ij softplus(x_ij) and, when dZ is not null, dZ[i] = 2 Σ_j sigmoid(x_ij) z_j, from
 *   one tiled pass over Z Zᵀ on the exact-fp32 matrix cores; a wave owns ctgcn_vae_nll_tile() rows and walks every column tile, rows
 *   and columns beyond n masked out of both sums.  Z [n, d] fp32 with row stride ldz; any d >= 1 (above 128 one launch per 128
 *   columns of dZ).
 * ctgcn_vae_nll_entries_f32: per stored entry e = (i, j) of the CSR, coef[e] = a_e (−posw_m1 sigmoid(−x_e) − 1), the derivative of the
 *   entry's term by x_e, and, when loss is not null, loss[0] = Σ_e a_e (posw_m1 softplus(−x_e) − x_e) in fp64.  dZ += C Z + Cᵀ Z with
 *   C the CSR holding coef is then the plain aggregation (ctgcn_gcn_conv_fwd_f32) over the CSR and its transpose.
 * workspace: ctgcn_vae_nll_workspace_bytes(n, nnz) bytes, 8-byte aligned (the entries call needs it only with loss).  Returns
 * CTGCN_E_INVALID for null pointers and bad sizes, CTGCN_E_WORKSPACE for a workspace that is too small; n = 0 or nnz = 0 writes
 * nothing.  No atomics: partial sums are fp64 and added in a fixed order, repeated calls are bit-identical.
 */
int32_t ctgcn_vae_nll_tile(void);
size_t ctgcn_vae_nll_workspace_bytes(int64_t n, int64_t nnz);
int ctgcn_vae_nll_dense_f32(int64_t n, int32_t d, const float *Z, int64_t ldz, float *dZ, int64_t lddz, double *loss, void *workspace,
                            size_t workspace_bytes, void *stream);
int ctgcn_vae_nll_entries_f32(int64_t n, int64_t nnz, int32_t d, const int32_t *row_ptr, const int32_t *col, const float *val,
                              const float *Z, int64_t ldz, double posw_m1, float *coef, double *loss, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- fused gathers of the VGRNN baseline (ctgcn_vgrnn.hip; reference baseline/vgrnn.py:380-397, :497-508) over a normalised CSR, on
 * the row-gather scaffold of ctgcn_gcn_conv_fwd_f32 (same long-row arguments and workspace rule, sized for the gathered width).  Every
 * result is [n, width] fp32 with row stride width; inputs have unit column stride and the given row strides.
 * ctgcn_ggru_gates_fwd_f32: [g_z | g_r | g_c] = Â U + bias with U [n, 3 hid] and bias [3 hid] or null;
 *   z = σ(g_z), r = σ(g_r), q = r ∘ h, c = g_c.
 * ctgcn_ggru_blend_fwd_f32: h_tilde = tanh(c + Â V) with V [n, hid]; h_new = z ∘ h + (1 − z) ∘ h_tilde.
 * ctgcn_vgrnn_heads_fwd_f32: [g_m | g_s] = Â S + bias with S [n, 2 out] and bias [2 out] or null; mean = g_m,
 *   std = softplus(g_s) (g_s above 20 is passed through, as F.softplus does), z = mean + noise ∘ std.
 * ctgcn_vgrnn_bwd_prep_f32: the one N x d pass of each backward.  G [n, segments x width] = the gradient in front of the gather, which the
 *   plain aggregation over the transposed CSR (ctgcn_gcn_conv_fwd_f32) then takes to the source; db [segments x width], when not null,
 *   = the column sums of G, per-block partial sums added in block order (workspace: ctgcn_gcn_conv_prep_workspace_bytes(n, segments x
 *   width) bytes, 16-byte aligned).  An incoming gradient that is null counts as zero.  x0, x1 are [n, width] with row stride width.
 *     mode 0 (gates, 3 segments): g = dz, dq, dc; s = z, r, h: G = [dz z (1 − z) | dq h r (1 − r) | dc], x0 = dh = dq r
 *     mode 1 (blend, 1 segment):  g0 = dh' (required); s = z, h, h_tilde: G = dh' (1 − z) (1 − h_tilde²), x0 = dz = dh' (h − h_tilde),
 *                                 x1 = dh = dh' z; no db
 *     mode 2 (heads, 2 segments): g = dmean, dstd, dz; s = std, noise: G = [dmean + dz | (dstd + dz noise) (1 − exp(−std))]
 * Returns CTGCN_E_INVALID for null pointers and bad sizes, CTGCN_E_UNSUPPORTED for more than 65535 long rows, CTGCN_E_WORKSPACE for a
 * workspace that is too small; 0 for n = 0.  No atomics; repeated calls are bit-identical.
 */
int ctgcn_vgrnn_bwd_prep_f32(int32_t mode, int64_t n, int32_t width, const float *g0, int64_t ldg0, const float *g1, int64_t ldg1,
                             const float *g2, int64_t ldg2, const float *s0, int64_t lds0, const float *s1, int64_t lds1, const float *s2,
                             int64_t lds2, float *G, int64_t ldG, float *x0, float *x1, float *db, void *workspace, size_t workspace_bytes,
                             void *stream);
int ctgcn_ggru_gates_fwd_f32(int64_t n, int32_t hid, const int32_t *row_ptr, const int32_t *col, const float *val, const float *U, int64_t ldu,
                             const float *bias, const float *h, int64_t ldh, float *z, float *r, float *q, float *c,
                             const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                             void *stream);
int ctgcn_ggru_blend_fwd_f32(int64_t n, int32_t hid, const int32_t *row_ptr, const int32_t *col, const float *val, const float *V, int64_t ldv,
                             const float *c, int64_t ldc, const float *z, int64_t ldz, const float *h, int64_t ldh, float *h_new,
                             float *h_tilde, const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace,
                             size_t workspace_bytes, void *stream);
int ctgcn_vgrnn_heads_fwd_f32(int64_t n, int32_t out, const int32_t *row_ptr, const int32_t *col, const float *val, const float *S, int64_t lds,
                              const float *bias, const float *noise, int64_t ldnoise, float *mean, float *std_out, float *z,
                              const int32_t *long_rows, int32_t n_long, int32_t long_threshold, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ---- row-selected passes of the DynGEM and DynAE baselines (ctgcn_dyngem.hip; reference baseline/dynGEM.py, baseline/dynAE.py) over a
 * window of snapshots stacked into one CSR: row t N + v is row v of snapshot t, columns are node ids, int32 indices, fp32 values.
 * ctgcn_rowsel_conv_fwd_f32: Y[b] = epi(bias + Σ_{s < slots} Σ_{e ∈ row idx[b][s]} val[e] S[s col_stride + col[e]]) for b < n: the first
 *   Linear of an MLP over dense adjacency rows, as a gather.  idx [n][slots] holds stacked row ids, -1 an empty row; epi 0 none,
 *   1 ReLU; Y [n, d] with row stride ldy, S with row stride lds, bias [d] or null; 1 <= slots <= ctgcn_rowsel_max_slots().  On the
 *   row-gather scaffold of ctgcn_gcn_conv_fwd_f32 with batch positions in the role of rows: a position's entries are those of its
 *   rows, slot after slot; long_pos lists the positions with more than long_threshold entries, cut into pieces by the same rule and
 *   with the same workspace rule.  The caller keeps every idx below the CSR's row count and s col_stride + col inside S.
 * ctgcn_rowsel_bucket_f32: out[r] = Σ G[inv_pos[k]] over inv_ptr[r] <= k < inv_ptr[r + 1], in that order, for r < rows; a row
 *   without positions is written as zeros.  With inv the inverted index of one slot of idx (per stacked row its batch positions,
 *   ascending), dS of that slot is the plain aggregation (ctgcn_gcn_conv_fwd_f32) of out over the transposed stack.
 * ctgcn_wrecon_loss_f32: with p = relu ? max(z, 0) : z and the stored entries (j, v), v != 0, of row tgt[b] (-1: none),
 *     l_b = (Σ_j p_bj² + Σ_stored (β² (p_bj − v)² − p_bj²)) / div_b,   loss[0] = scale Σ_b l_b   (fp32, device)
 *   which is Σ_j ((p_bj − x_bj) pen_bj)² / div_b for the dense target row x and pen = β where x != 0, 1 elsewhere.  div is indexed
 *   by stacked row id (div_b = div[tgt[b]], 0 for tgt -1) or null for 1.  dZ, when not null, receives d loss / d Z (zero where the
 *   ReLU was inactive) and may be Z itself.  ent_ptr [n + 1] (int64) are the running sums of the targets' row lengths and entries =
 *   ent_ptr[n]: z at the stored columns is staged there before the sweep of the row may overwrite it; a row whose ent_ptr does not
 *   match its length gets a NaN loss.  A row's sweep and its correction run in one workgroup, in that order; row sums are fp64 and
 *   added in row order; the float4 and the scalar form (width, strides, bases) add the same numbers in the same order, so the loss
 *   with and without dZ is the same bit pattern.  workspace: ctgcn_wrecon_loss_workspace_bytes(n, entries) bytes, 16-byte aligned.
 * Returns CTGCN_E_INVALID for null pointers and bad sizes, CTGCN_E_UNSUPPORTED for more than 65535 long positions, CTGCN_E_WORKSPACE for
 * a workspace that is too small; n = 0 writes nothing (the loss call: loss[0] = 0).  No atomics; repeated calls are bit-identical.
 */
int32_t ctgcn_rowsel_max_slots(void);
int ctgcn_rowsel_conv_fwd_f32(int64_t n, int32_t slots, int32_t d, const int32_t *idx, const int32_t *row_ptr, const int32_t *col,
                              const float *val, const float *S, int64_t lds, int64_t col_stride, const float *bias, int32_t epi, float *Y,
                              int64_t ldy, const int32_t *long_pos, int32_t n_long, int32_t long_threshold, void *workspace,
                              size_t workspace_bytes, void *stream);
int ctgcn_rowsel_bucket_f32(int64_t rows, int32_t d, const int32_t *inv_ptr, const int32_t *inv_pos, const float *G, int64_t ldg, float *out,
                            int64_t ldout, void *stream);
size_t ctgcn_wrecon_loss_workspace_bytes(int64_t n, int64_t entries);
int ctgcn_wrecon_loss_f32(int64_t n, int64_t width, const float *Z, int64_t ldz, const int32_t *tgt, const int64_t *ent_ptr, int64_t entries,
                          const int32_t *row_ptr, const int32_t *col, const float *val, double beta, const float *div, double scale,
                          int32_t relu, float *dZ, int64_t lddz, float *loss, void *workspace, size_t workspace_bytes, void *stream);

/* ---- one time step of an LSTM layer of any width (ctgcn_lstmcell.hip; the DynRNN and DynAERNN baselines, reference baseline/dynRNN.py,
 * baseline/dynAERNN.py).  The products with W_ih and W_hh are the caller's GEMMs; these are the element-wise passes between them.
 * B rows of hidden width H; a gate operand is [B, 4 H] in torch's order i, f, g, o, a state operand [B, H]; every operand has its own
 * row stride, so a step may be a slice of a [B, L, .] or [L, B, .] tensor.
 * ctgcn_lstm_cell_fwd_f32: z = gi + gh + bias; i, f, o = σ(z), g = tanh(z); c = f c_prev + i g; h = o tanh(c).  gh null: no recurrent
 *   term (step 0, h_{-1} = 0); bias [4 H] or null; c_prev null: zero.  Writes h, c and, unless gates is null (inference), the four
 *   activated gates.  gates may be gi itself.
 * ctgcn_lstm_cell_bwd_f32: from the saved activated gates, c of the step and c_prev (null at step 0: zero), with dh = dh_out + dh_rec
 *   (the gradient from the layer above, and dgates_{t+1} W_hh from the caller's GEMM; either may be null) and dc = dh o (1 − tanh² c) +
 *   dc_next (null: zero), writes the pre-activation gate gradients dgates = (dc g i (1 − i), dc c_prev f (1 − f), dc i (1 − g²),
 *   dh tanh(c) o (1 − o)) and, unless dc_prev is null, dc_prev = dc f.  dc_prev may be dc_next itself; tanh(c) is recomputed.
 * Every element of every operand is read once and written once.  16-byte accesses when H and every row stride are multiples of 4
 * and every base is 16-byte aligned (the float4 rule of the gathers), scalar ones otherwise; 64-bit element indices; no atomics,
 * repeated calls are bit-identical; σ and tanh are exact at saturation (0, 1, ±1 for |z| >= 100, never NaN).
 * Returns CTGCN_E_INVALID for B outside [0, 2^31), H outside [1, 2^29), a row stride below the operand's width and a null gi, h, c
 * (forward) or gates, c, dgates (backward); B = 0 returns CTGCN_OK before any pointer check.
 */
int ctgcn_lstm_cell_fwd_f32(int64_t B, int32_t H, const float *gi, int64_t ldgi, const float *gh, int64_t ldgh, const float *bias,
                            const float *c_prev, int64_t ldcp, float *h, int64_t ldh, float *c, int64_t ldc, float *gates, int64_t ldg,
                            void *stream);
int ctgcn_lstm_cell_bwd_f32(int64_t B, int32_t H, const float *gates, int64_t ldg, const float *c, int64_t ldc, const float *c_prev,
                            int64_t ldcp, const float *dh_out, int64_t lddo, const float *dh_rec, int64_t lddr, const float *dc_next,
                            int64_t lddn, float *dgates, int64_t lddg, float *dc_prev, int64_t lddp, void *stream);

/* ---- one time step of a GRU layer of any width (ctgcn_grucell.hip; ops.gru_layer: the core-axis and the temporal RNN of CTGCN, CGCN
 * and GCRN at hidden widths other than 128).  The products with W_ih and W_hh are the caller's GEMMs; these are the element-wise
 * passes between them.  B rows of hidden width H; a gate operand is [B, 3 H] in torch's order r, z, n, a state operand [B, H]; every
 * operand has its own row stride, so a step may be a slice of a [B, L, .] or [L, B, .] tensor.
 * ctgcn_gru_cell_fwd_f32: r = σ(gi_r + gh_r + b_hr), z = σ(gi_z + gh_z + b_hz), q = gh_n + b_hn, n = tanh(gi_n + r q),
 *   h = (1 − z) n + z h_prev.  gi = x W_ihᵀ + b_ih and gh = h_prev W_hhᵀ come from the caller; gh null: no recurrent term (step 0,
 *   h_{-1} = 0); b_hh [3 H] or null; h_prev null: zero.  Writes h and, unless gates and q are both null (inference), the activated
 *   gates (r, z, n) [B, 3 H] and q [B, H]: what the backward reads.  acc not null: the running sum over the steps, acc = h with
 *   acc_init != 0 (the first step: acc's old contents are not read) and acc += h otherwise.  gates may be gi itself and h may be
 *   h_prev itself; acc and q are memory of their own.
 * ctgcn_gru_cell_bwd_f32: from the saved gates and q of the step and h_prev (null at step 0: zero), with dh = dh_out + dh_rec (the
 *   gradient from above, and the complete dh_prev of step t + 1; either may be null), dn = dh (1 − z), dz = dh (h_prev − n),
 *   da_n = dn (1 − n²), da_z = dz z (1 − z), da_r = da_n q r (1 − r): writes dgi = (da_r, da_z, da_n), unless dgh is null
 *   dgh = (da_r, da_z, da_n r), and unless dh_prev is null the direct part dh z of dh_prev; the caller's GEMM adds dgh W_hh to it.
 *   dh_prev may be dh_rec itself, and dgi may be gates itself (when the saved gates are not needed again).
 * Every element of every operand is read once and written once.  16-byte accesses when H and every row stride are multiples of 4
 * and every base is 16-byte aligned (the float4 rule of the gathers), scalar ones otherwise; 64-bit element indices; no LDS, no
 * atomics, repeated calls are bit-identical; σ and tanh are exact at saturation (0, 1, ±1 for |z| >= 100, never NaN).
 * Returns CTGCN_E_INVALID for B outside [0, 2^31), H outside [1, 2^29), a row stride below the operand's width, a null gi, h
 * (forward) or gates, q, dgi (backward), and gates without q or q without gates (forward); B = 0 returns CTGCN_OK before any pointer
 * check.
 */
int ctgcn_gru_cell_fwd_f32(int64_t B, int32_t H, const float *gi, int64_t ldgi, const float *gh, int64_t ldgh, const float *b_hh,
                           const float *h_prev, int64_t ldhp, float *h, int64_t ldh, float *gates, int64_t ldg, float *q, int64_t ldq,
                           float *acc, int64_t ldacc, int32_t acc_init, void *stream);
int ctgcn_gru_cell_bwd_f32(int64_t B, int32_t H, const float *gates, int64_t ldg, const float *q, int64_t ldq, const float *h_prev,
                           int64_t ldhp, const float *dh_out, int64_t lddo, const float *dh_rec, int64_t lddr, float *dgi, int64_t lddgi,
                           float *dgh, int64_t lddgh, float *dh_prev, int64_t lddp, void *stream);

/* ---- the fp64 linear algebra of the TIMERS baseline (ctgcn_timers.hip; reference baseline/timers.py): the passes of a block
 * eigensolver on a CSR operator (ops.sym_topk), the edge-gather loss, TRIP and the restart bound.  Everything is double, row-major
 * with leading dimensions in elements; CSR as in ctgcn_spmm_csr_f32 (int32 row_ptr[n + 1] and col).
 * ctgcn_spmm_csr_f64: Y[n, b] = A·X, or Y += A·X with accumulate != 0; each row's sum in CSR order.  Y must not overlap X.
 * ctgcn_tsgemm_tn_f64: G[b1, b2] (dense, row stride b2) = Xᵀ·Y over n rows, X [n, b1], Y [n, b2] (Y may be X).  n = 0 zeroes G.
 *   workspace: ctgcn_tsgemm_tn_workspace_bytes (0 up to 512 rows: one run, no partials).
 * ctgcn_tsgemm_nn_f64: Y[n, b2] = X[n, b1]·C[b1, b2]; colsq (device double[b2], or null) = the column sums of squares of Y.  Y must
 *   not overlap X.  workspace: ctgcn_tsgemm_nn_workspace_bytes, read only with colsq.
 * ctgcn_timers_obj_f64: over the stored entries (r, c, s) of a CSR matrix, with d = ⟨U_r, V_c⟩ over k columns: out[0] = Σ s² and
 *   out[1] = Σ s·d; with s_old (a second value array on the same pattern) out[0] = Σ (s_old + s − d)² − (s_old − d)² instead.
 *   workspace: ctgcn_timers_obj_workspace_bytes.
 * Limits: 1 <= b1, b2 <= 512 in the two products (b1 <= 1024 in ctgcn_tsgemm_nn_f64, whose X may be two blocks side by side), else
 * CTGCN_E_UNSUPPORTED; n < 2^31 in the two CSR passes.
 * Returns CTGCN_E_INVALID for bad sizes, a leading dimension below its width and null pointers, CTGCN_E_WORKSPACE for a workspace
 * that is too small; n = 0 returns CTGCN_OK before any pointer check.  No float atomics: per-block partials summed in a fixed order,
 * their count a function of the sizes alone, so repeated calls are bit-identical.
 */
int ctgcn_spmm_csr_f64(int64_t n_rows, int32_t b, const int32_t *row_ptr, const int32_t *col_idx, const double *val, const double *X,
                       int64_t ldx, double *Y, int64_t ldy, int accumulate, void *stream);
size_t ctgcn_tsgemm_tn_workspace_bytes(int64_t n, int32_t b1, int32_t b2);
int ctgcn_tsgemm_tn_f64(int64_t n, int32_t b1, int32_t b2, const double *X, int64_t ldx, const double *Y, int64_t ldy, double *G,
                        void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_tsgemm_nn_workspace_bytes(int64_t n, int32_t b2);
int ctgcn_tsgemm_nn_f64(int64_t n, int32_t b1, int32_t b2, const double *X, int64_t ldx, const double *C, int64_t ldc, double *Y,
                        int64_t ldy, double *colsq, void *workspace, size_t workspace_bytes, void *stream);
size_t ctgcn_timers_obj_workspace_bytes(int64_t n, int32_t k);
int ctgcn_timers_obj_f64(int64_t n, int32_t k, const int32_t *row_ptr, const int32_t *col, const double *s, const double *s_old,
                         const double *U, int64_t ldu, const double *V, int64_t ldv, double *out, void *workspace, size_t workspace_bytes,
                         void *stream);

size_t ctgcn_workspace_bytes(int op, int64_t n, int64_t nnz, int32_t d, int32_t K);

#ifdef __cplusplus
}
#endif
#endif /* CTGCN_HIP_H */
