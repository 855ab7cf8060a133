/*
 * mmrec_hip.h -- C ABI of libmmrec_hip.so, the MI355X (gfx950) implementation of the MMRec hot path.
 *
 * The reference (enoche/MMRec) has no native layer and no FFI: its hot path is a set of stock torch
 * calls inside each model class.  Each entry point below replaces one of
 * those call sites; the citation after "replaces" is the reference file:line under
 * /root/reference/src.  A maintainer binds them with ctypes (see INTEGRATION.md and
 * mmrec_amd/_lib.py), which is what a Python reference would use as its FFI.
 *
 * Contract:
 *   - plain pointers and sizes only; no torch types; all pointers are DEVICE pointers unless a
 *     parameter is documented as host;
 *   - every call ENQUEUES work on `stream` (a hipStream_t passed as void*) and returns at once; it
 *     never synchronises, never allocates or frees device memory and keeps no global mutable state
 *     (re-entrant).  The caller owns every buffer, including workspaces whose size the matching
 *     *_workspace_bytes() call reports;
 *   - return value: 0 on success, otherwise a hipError_t value (mmrec_error_string() names it), or
 *     MMREC_ERR_* below for argument errors detected on the host;
 *   - row-major contiguous fp32 matrices; int32 CSR indices; int64 ids where the reference hands
 *     over torch.LongTensor ids (batches, masks, top-K output).
 */
#ifndef MMREC_HIP_H
#define MMREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMREC_ABI_VERSION 16
#define MMREC_EMB_DIM 64 /* embedding_size the SpMM / BPR / top-K kernels are specialised for (overall.yaml:16) */

#define MMREC_ERR_BAD_ARG 10001      /* null pointer / negative size / unsupported d or k */
#define MMREC_ERR_UNSUPPORTED 10002  /* shape outside what the kernel is built for */

typedef void* mmrec_stream_t; /* hipStream_t */

int mmrec_abi_version(void);
const char* mmrec_error_string(int err);

/* ------------------------------------------------------------------------------------------------
 * P2  sparse propagation  Y = alpha * A X (+ beta * Z), optional fused running layer sum.
 * replaces: torch.sparse.mm(adj, ego) -- models/freedom.py:167,172  bm3.py:90  layergcn.py:131
 *           lightgcn.py:120  lattice.py:169,188  common/encoders.py:99,122 ; and the
 *           stack(...).mean(dim=1) epilogue -- freedom.py:175-176  bm3.py:92-93  lightgcn.py:122-123.
 *
 * A is CSR (rowptr[n_rows+1], colidx[nnz], vals[nnz]) with n_rows local rows whose column ids index
 * rows of X (any number of X rows; a rank of a row-sharded graph passes its row block here).
 * d must be a multiple of 64, at most 384 (64 for the d = 64 graph models; 256 / 384 for MMGCN's
 * modality layers) -- or 8, 16 or 32: ONE FEATURE SLICE of a 64-wide table (X, Y, Z, acc_* are [rows, d] row-major slices;
 * the feature-sliced multi-GPU layout, where a rank owns 64 / P columns of every table and the whole graph: a column's
 * sum is the d = 64 launch's, operation for operation, so the P slices ARE the columns of the single-GPU result).
 * Rows are summed in CSR order, a fixed order that does not depend on how rows are
 * partitioned over GPUs, so sharded == single-GPU bit for bit.
 *
 * Rows longer than `long_row_threshold` are not handled by the row kernel; the caller lists them
 * in a plan (host-built, see mmrec_spmm_plan_*): long_rows[n_long] (row ids, ascending),
 * long_chunk_ptr[n_long+1] (prefix sum of ceil(deg / MMREC_SPMM_CHUNK) per long row).  Each chunk
 * is reduced by one workgroup into `partials` (n_chunks x d fp32 workspace) and the chunks of a row
 * are then summed in order -- deterministic, no float atomics.  partials = n_chunks * d floats.
 * long_tickets (ABI 7; may be NULL): n_long int32 counters, ZERO before the first call and left at zero by every call.
 * With them, a multi-chunk row is finished inside the launch (the chunk block that arrives last sums the partials, in the
 * same order: same bits) instead of in a second launch, at every graph size (Amazon-Baby: 18.5 -> 15.4 us per layer; config 5:
 * the 18-us second launch and its gap).  Without them (NULL) the second launch runs.  One graph's tickets / partials must not
 * be used by two launches at the same time.
 *
 * Epilogue per row r (y = alpha * sum + beta * Z[r], Z may be NULL):
 *      Y[r] = y                         (Y may be NULL when only the running sum is wanted)
 *      acc_out[r] = acc_scale * (acc_in[r] + y)      (when acc_out != NULL; acc_in may alias acc_out)
 * Y and acc_out must not be X (other rows still gather from it): MMREC_ERR_BAD_ARG.
 * which is how the LightGCN layer mean (1/(L+1) * sum_l E_l) is accumulated without a stack+mean pass.
 * ---------------------------------------------------------------------------------------------- */
#ifndef MMREC_SPMM_CHUNK
#define MMREC_SPMM_CHUNK 512            /* nnz per long-row chunk (one workgroup) */
#endif
#define MMREC_SPMM_LONG_ROW_DEFAULT 32  /* long_row_threshold of HBM-sized graphs; cache-resident ones (<= 2^18 columns) run
                                          * 30 % faster with 16: mmrec_amd/hip_ops.py default_long_row_threshold */

int mmrec_spmm_csr_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals,
                       const float* X, float* Y, const float* Z, const float* acc_in, float* acc_out,
                       int32_t n_rows, int32_t d, float alpha, float beta, float acc_scale,
                       int32_t long_row_threshold, const int32_t* long_rows,
                       const int32_t* long_chunk_ptr, int32_t n_long, int32_t n_chunks,
                       float* partials, int32_t* long_tickets, mmrec_stream_t stream);

/* The same product at LISTED rows only (ABI 10): Y[i] = (A X)[rows[i]] + Z[rows[i]] (z_compact = 0; Z may be NULL) or
 * + Z[i] (z_compact = 1: Z is [n_list, d] like Y), i < n_list, rows int64 (duplicates allowed), Y [n_list, d] compact,
 * d = 8 / 16 / 32 / 64.  For the training step of a model that consumes a propagated table at its batch rows only -- FREEDOM's
 * item-item layer, freedom.py:173-177 read at :197-199: 4096 of 500,000 rows at config 5.
 * Bits: those of mmrec_spmm_csr_f32 with the same long_row_threshold for every row that does not span several chunks
 * (n_chunks == n_long in the graph's plan; callers keep the full launch otherwise).
 * mmrec_spmm_push_rows_f32 is the transposed product of the listed rows without a transposed graph:
 * dX[c] += A[r, c] * g_scale * G[i] over the nonzeros (r, c) of the listed rows r = rows[i], and dZ[r] += g_scale * G[i]
 * (either may be NULL; dZ may alias dX); one workgroup per listed row; fp32 atomics into caller-zeroed / accumulating buffers,
 * so the order of the sums differs from a pull launch's in the last ulp (as the sampled-scoring backward's scatters do). */
int mmrec_spmm_rows_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X,
                        const float* Z, int32_t z_compact, const int64_t* rows, int32_t n_list, int32_t d,
                        int32_t long_row_threshold, float* Y, mmrec_stream_t stream);
/* ABI 12: the same for ANY listed row of a d = 64 graph, rows spanning several chunks included (one workgroup per such listed
 * row sums its chunks in the full launch's order: its bits).  max_row_chunks: the largest number of 512-nonzero chunks a row of
 * the graph's long-row plan spans (1: identical to mmrec_spmm_rows_f32; up to 480 = 245,760 nonzeros; more: MMREC_ERR_UNSUPPORTED).
 * A listed row that spans more chunks than max_row_chunks (a value smaller than the plan's) is not computed: its Y row is
 * written as quiet NaN.
 * For a training step that reads the LAST user-item layer (freedom.py:169-177) at its batch rows only: popular items are in
 * every batch and their rows span dozens of chunks. */
int mmrec_spmm_rows_any_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X,
                            const float* Z, int32_t z_compact, const int64_t* rows, int32_t n_list, int32_t d,
                            int32_t long_row_threshold, int32_t max_row_chunks, float* Y, mmrec_stream_t stream);
int mmrec_spmm_push_rows_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* G,
                             float g_scale, const int64_t* rows, int32_t n_list, int32_t d, float* dX, float* dZ,
                             mmrec_stream_t stream);

/* One LayerGCN layer in one launch (layergcn.py:131-135): y = A x ; w[row] = cosine_similarity(y[row], ego[row]) with
 * eps 1e-8 per norm ; scaled = w * y (the next layer's input) ; acc_out = acc_in + scaled (acc_in NULL: acc_out = scaled;
 * acc_out NULL: no sum).  Y (the unscaled product, needed by the backward) may be NULL.  d must be 64.  Plan arguments
 * as in mmrec_spmm_csr_f32.  Results are bit-identical to mmrec_spmm_csr_f32 followed by mmrec_cos_scale_fwd_f32. */
int mmrec_spmm_csr_f32_layergcn(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X,
                                float* Y, const float* ego, float* scaled, float* w, const float* acc_in,
                                float* acc_out, int32_t n_rows, int32_t d, int32_t long_row_threshold,
                                const int32_t* long_rows, const int32_t* long_chunk_ptr, int32_t n_long,
                                int32_t n_chunks, float* partials, int32_t* long_tickets, mmrec_stream_t stream);
/* Row schedule of a large graph (additive to ABI 16).  mmrec_spmm_csr_sched_f32 is mmrec_spmm_csr_f32 with the row blocks
 * visiting the SHORT rows (nnz <= long_row_threshold, empty rows included) in the order of a caller-built schedule instead of
 * row-id order: slot i visits row sched_row[i], whose (column, value) entries are sched_col / sched_val[sched_span[2 i] ..
 * sched_span[2 i + 1]) -- a packed copy of the row's CSR segment, entries in CSR order.  sched_row must list every short row
 * exactly once and no long row (n_short of them); long rows are served from the CSR by the chunk blocks as before.  d = 64 k
 * only (k <= 6; the feature slices keep mmrec_spmm_csr_f32).  Every row's sum runs over the same entries in the same order:
 * the results are BIT-IDENTICAL to mmrec_spmm_csr_f32 for any valid schedule; only the order in which rows meet in the
 * caches changes (rows that share a cold column side by side: that column is fetched past L2 once per block, not once per
 * row).  mmrec_spmm_csr_sched_f32_layergcn is the same twin of mmrec_spmm_csr_f32_layergcn.
 * mmrec_spmm_row_keys writes, for every row, the sort key such a schedule is built from: key[row] = among the row's columns
 * with col_degree <= key_deg_max the one with the largest col_degree (first in row order among equals), key_degree[row] =
 * that degree; -1 and 0 for a row without such a column, an empty row, or a long row.  col_degree: int32 [n_cols]. */
int mmrec_spmm_csr_sched_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X, float* Y,
                             const float* Z, const float* acc_in, float* acc_out, int32_t n_rows, int32_t d, float alpha,
                             float beta, float acc_scale, int32_t long_row_threshold, const int32_t* long_rows,
                             const int32_t* long_chunk_ptr, int32_t n_long, int32_t n_chunks, float* partials,
                             int32_t* long_tickets, const int32_t* sched_row, const int32_t* sched_span,
                             const int32_t* sched_col, const float* sched_val, int32_t n_short, mmrec_stream_t stream);
int mmrec_spmm_csr_sched_f32_layergcn(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X,
                                      float* Y, const float* ego, float* scaled, float* w, const float* acc_in,
                                      float* acc_out, int32_t n_rows, int32_t d, int32_t long_row_threshold,
                                      const int32_t* long_rows, const int32_t* long_chunk_ptr, int32_t n_long,
                                      int32_t n_chunks, float* partials, int32_t* long_tickets, const int32_t* sched_row,
                                      const int32_t* sched_span, const int32_t* sched_col, const float* sched_val,
                                      int32_t n_short, mmrec_stream_t stream);
int mmrec_spmm_row_keys(const int32_t* rowptr, const int32_t* colidx, const int32_t* col_degree, int32_t n_rows,
                        int32_t long_row_threshold, int32_t key_deg_max, int32_t* key, int32_t* key_degree,
                        mmrec_stream_t stream);

/* Edge dropout inside the product (common/encoders.py:77-103: sparse_dropout of the normalised adjacency, drawn per batch).
 * ADDITIVE to ABI 16: two new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * The mask is ONE BIT PER CSR ENTRY in the order of the CSR the launch runs on: entry k is bit (k & 31) of the 32-bit word
 * keep_bits[k >> 5] ((nnz + 31) / 32 words); a set bit means kept.
 * mmrec_spmm_csr_masked_f32 is mmrec_spmm_csr_f32 -- arguments, plan (the FULL graph's: thresholds, chunk boundaries, tickets,
 * the two-launch finish without them), epilogue -- on the matrix in which entry k has the value vals[k] * val_scale (one fp32
 * multiply) if its bit is set and is ABSENT otherwise: its source row is never gathered.  A row's kept entries are added in
 * CSR order at the positions the unmasked launch adds them, so
 *   - with every bit set and val_scale = 1 the result is bit-identical to mmrec_spmm_csr_f32;
 *   - for finite X it equals, as numbers, mmrec_spmm_csr_f32 on the value vector whose dropped entries are +0;
 *   - a dropped entry whose source row holds inf / NaN contributes nothing (the zero-valued form gives NaN).
 * d: a multiple of 64 up to 384; the 8 / 16 / 32-column slices are not served (MMREC_ERR_UNSUPPORTED).
 * mmrec_edge_keep_bits packs a keep vector (one byte per entry, nonzero = kept, the caller's edge order) for up to two entry
 * orders in one launch: bit j of bits_x = keep[perm_x[j]] (perm_x int64 [n_edges], NULL = identity; bits_b NULL = one
 * output only).  Bits at positions >= n_edges of the last word are written as zero.  n_edges = 0 launches nothing. */
int mmrec_spmm_csr_masked_f32(const int32_t* rowptr, const int32_t* colidx, const float* vals, const float* X, float* Y,
                              const float* Z, const float* acc_in, float* acc_out, int32_t n_rows, int32_t d, float alpha,
                              float beta, float acc_scale, int32_t long_row_threshold, const int32_t* long_rows,
                              const int32_t* long_chunk_ptr, int32_t n_long, int32_t n_chunks, float* partials,
                              int32_t* long_tickets, const uint32_t* keep_bits, float val_scale, mmrec_stream_t stream);
int mmrec_edge_keep_bits(const uint8_t* keep, int64_t n_edges, const int64_t* perm_a, uint32_t* bits_a,
                         const int64_t* perm_b, uint32_t* bits_b, mmrec_stream_t stream);
/* Host-side plan helpers (pure CPU, rowptr is a HOST pointer).  count: returns n_long and n_chunks;
 * fill: writes long_rows[n_long] and long_chunk_ptr[n_long+1] (host arrays the caller copies to the
 * device).  partials workspace = n_chunks * d * 4 bytes (d: the row width of the SpMM call). */
int mmrec_spmm_plan_count(const int32_t* rowptr_host, int32_t n_rows, int32_t long_row_threshold,
                          int32_t* n_long, int32_t* n_chunks);
int mmrec_spmm_plan_fill(const int32_t* rowptr_host, int32_t n_rows, int32_t long_row_threshold,
                         int32_t* long_rows, int32_t* long_chunk_ptr);

/* LayerGCN per-layer re-weighting: w[r] = cos(E[r], Ego[r]) with eps 1e-8 (torch >= 2 semantics:
 * each norm clamped), Out[r] = w[r] * E[r]; optional running sum Acc[r] += Out[r].
 * replaces: F.cosine_similarity + einsum('a,ab->ab') -- models/layergcn.py:132-134 (+ the layer sum :136).
 * Backward: given dOut (gradient w.r.t. Out, already including the layer-sum branch), E, Ego, w:
 *   dE, dEgo_add (accumulated into dEgo).  d must be 64. */
int mmrec_cos_scale_fwd_f32(const float* E, const float* Ego, float* Out, float* w, float* acc,
                            int32_t n_rows, int32_t d, mmrec_stream_t stream);
int mmrec_cos_scale_bwd_f32(const float* dOut, const float* E, const float* Ego, const float* w,
                            float* dE, float* dEgo_accum, int32_t n_rows, int32_t d,
                            mmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * P4  sampled scoring: fused gather - dot - (log)sigmoid and its scatter-add backward.
 * replaces: FREEDOM.bpr_loss freedom.py:180-187 (variant LOGSIG, mean) ; LayerGCN.bpr_loss
 *           layergcn.py:140-152 (LOGSIG, sum) ; BPRLoss common/loss.py:33-35 (GAMMA, mean; used by
 *           vbpr.py:94, lightgcn.py:142) ; the row gathers ua[users], ia[pos], ia[neg]
 *           freedom.py:197-199.
 * U [n_u, d], P and N tables [n_i, d] (P and N may be the same table; row strides = d; d a multiple
 * of 64: 64 for the graph models, 128 for VBPR's cat(id, visual) embeddings vbpr.py:71).
 * ids: users[B], pos[B], neg[B] int64.  Outputs: loss_out[1] = scale * sum_b l_b  (scale = 1/B for the
 * mean variants, 1 for sum), coef[B] = d l_b / d x_b  (x_b = <u,p> - <u,n>), for the backward.
 * workspace: mmrec_bpr_workspace_bytes(B).  The loss reduction is a fixed-order tree (deterministic).
 * Backward: dU[users[b]] += g*coef[b]*(p - n) ; dP[pos[b]] += g*coef[b]*u ; dN[neg[b]] -= g*coef[b]*u
 * with g = *grad_scalar (device pointer, upstream gradient of the scalar loss) * scale;
 * duplicate ids are combined with fp32 atomics (order-dependent in the last ulp).
 * ---------------------------------------------------------------------------------------------- */
#define MMREC_BPR_LOGSIG 0 /* l = -logsigmoid(x) */
#define MMREC_BPR_GAMMA 1  /* l = -log(1e-10 + sigmoid(x)) */

size_t mmrec_bpr_workspace_bytes(int32_t batch);
int mmrec_bpr_fwd_f32(const float* U, const float* P, const float* N, const int64_t* users,
                      const int64_t* pos, const int64_t* neg, int32_t batch, int32_t d,
                      int32_t variant, float scale, float* loss_out, float* coef, void* workspace,
                      mmrec_stream_t stream);
int mmrec_bpr_bwd_f32(const float* U, const float* P, const float* N, const int64_t* users,
                      const int64_t* pos, const int64_t* neg, int32_t batch, int32_t d,
                      const float* coef, const float* grad_scalar, float scale, float* dU, float* dP,
                      float* dN, mmrec_stream_t stream);

/* The same loss on a COLUMN SLICE of the tables (feature-sliced multi-GPU layout, SURVEY.md 8e: a rank holds d / P = 8, 16
 * or 32 columns of every table; whole tables, d a multiple of 64, work too).  <u, p> and <u, n> of freedom.py:183-184 are sums
 * over the ranks of partial dot products: mmrec_bpr_dots_f32 writes dots[0..B) = <u, p>, dots[B..2B) = <u, n> over the
 * columns given; the caller sums `dots` over the ranks (one all-reduce of 2B floats per term), then
 * mmrec_bpr_loss_from_dots_f32 computes loss_out / coef from the sums exactly as mmrec_bpr_fwd_f32 does (same workspace
 * size), and mmrec_bpr_bwd_f32 takes that coef on the rank's own columns (d = 8 / 16 / 32 accepted there as well). */
int mmrec_bpr_dots_f32(const float* U, const float* P, const float* N, const int64_t* users,
                       const int64_t* pos, const int64_t* neg, int32_t batch, int32_t d, float* dots,
                       mmrec_stream_t stream);
int mmrec_bpr_loss_from_dots_f32(const float* dots, int32_t batch, int32_t variant, float scale,
                                 float* loss_out, float* coef, void* workspace, mmrec_stream_t stream);

/* Sum of squared L2 norms of gathered rows: out[0] = sum_b ||E[ids[b]]||^2 (fixed-order tree).
 * replaces the gathers + norms of EmbLoss / L2Loss -- common/loss.py:46-51,58-62 as used at
 * lightgcn.py:145-149, layergcn.py:154-161, vbpr.py:95.  Backward: dE[ids[b]] += coef * E[ids[b]]
 * (coef is a device scalar: 2*g for ||.||^2, g for 0.5||.||^2, g/||.|| for the unsquared norm). */
int mmrec_gather_sqnorm_fwd_f32(const float* E, const int64_t* ids, int32_t batch, int32_t d,
                                float* out, void* workspace, mmrec_stream_t stream);
int mmrec_gather_scale_add_bwd_f32(const float* E, const int64_t* ids, int32_t batch, int32_t d,
                                   const float* coef_scalar, float* dE, mmrec_stream_t stream);
/* ABI 14 -- the whole regulariser of a training step in one forward call (two launches) and one backward launch:
 *   out[0] = scale * sum_t f(S_t),  S_t = sum_b ||E[t][ids[t][b]]||^2,  mode 0: f = identity (the L2 regulariser on the
 *   batch's rows: layergcn.py:154-161, lattice.py:214-216), mode 1: f = sqrt (EmbLoss: common/loss.py:46-51 as used at
 *   vbpr.py:95, lightgcn.py:145-149); n_terms <= MMREC_ROWS_REG_MAX_TERMS, batch[t] rows per term, rows of d = 64 k floats.
 *   coef[t] (out, device) = the factor of the backward: dE[t][ids[t][b]] += g[0] * coef[t] * E[t][ids[t][b]] (fp32 atomics;
 *   two terms may name the same E / dE: the item table's positive and negative rows).  A term whose S_t is 0 gets coef 0 in
 *   mode 1, as torch.norm's backward does.  ids[t] NULL: rows 0 .. batch[t] - 1 of E[t] (a whole table: bm3.py:146's
 *   EmbLoss(u, i)).  E, ids, batch, dE are HOST arrays of n_terms entries (copied into the launch).
 *   Two terms' dE tables must be the SAME pointer or must not overlap (a whole table named by one term only is added without
 *   atomics).
 * replaces: the per-term mmrec_gather_sqnorm_fwd_f32 / mmrec_gather_scale_add_bwd_f32 calls and the ~20 elementwise
 * launches between them (a quarter of a LayerGCN / VBPR step at Amazon-Baby size). */
#define MMREC_ROWS_REG_MAX_TERMS 6
size_t mmrec_rows_reg_workspace_bytes(int32_t n_terms, int32_t max_batch);
int mmrec_rows_reg_fwd_f32(const float* const* E, const int64_t* const* ids, const int32_t* batch, int32_t n_terms, int32_t d,
                           int32_t mode, float scale, float* out, float* coef, void* workspace, mmrec_stream_t stream);
int mmrec_rows_reg_bwd_f32(const float* const* E, const int64_t* const* ids, const int32_t* batch, int32_t n_terms, int32_t d,
                           const float* coef, const float* g, float* const* dE, mmrec_stream_t stream);

/* ABI 14 -- several BPR terms over the SAME user rows in one forward call (two launches) and one backward launch:
 *   losses[t] = scale * sum_b loss(<U[users[b]], I[t][pos[t][b]]> - <U[users[b]], I[t][neg[t][b]]>)  (losses may be NULL),
 *   total[0] = sum_t w[t] * losses[t];  coef [n_terms][batch] as mmrec_bpr_fwd_f32's per term;  n_terms <= MMREC_BPR_MAX_TERMS.
 *   bwd: dU[users[b]] += c (p - n), dI[t][pos] += c u, dI[t][neg] -= c u with c = g[0] scale w[t] coef[t][b] (fp32 atomics; dU or
 *   any dI[t] may be NULL).  I, pos, neg, w, dI are HOST arrays of n_terms entries.
 * replaces: bpr_loss(id) + reg_weight * (bpr_loss(text) + bpr_loss(image)) of freedom.py:197-211 (per-term form:
 * mmrec_bpr_fwd_f32 / mmrec_bpr_bwd_f32 and the scalar launches that weight and add the three losses). */
#define MMREC_BPR_MAX_TERMS 4
size_t mmrec_bpr_multi_workspace_bytes(int32_t n_terms, int32_t batch);
int mmrec_bpr_multi_fwd_f32(const float* U, const int64_t* users, const float* const* I, const int64_t* const* pos,
                            const int64_t* const* neg, const float* w, int32_t n_terms, int32_t batch, int32_t d, int32_t variant,
                            float scale, float* total, float* losses, float* coef, void* workspace, mmrec_stream_t stream);
int mmrec_bpr_multi_bwd_f32(const float* U, const int64_t* users, const float* const* I, const int64_t* const* pos,
                            const int64_t* const* neg, const float* w, int32_t n_terms, int32_t batch, int32_t d, const float* coef,
                            const float* grad_scalar, float scale, float* dU, float* const* dI, mmrec_stream_t stream);

/* ABI 14 -- several mean-cosine terms in one forward call (two launches) and one backward launch:
 *   out[0] = sum_t w[t] * mean_b cos(X[t][ix[t][b]], Y[t][iy[t][b]])   (ix[t] / iy[t] NULL: row b; Y constant; F.cosine_similarity's
 *   1e-8 clamp; n_terms <= MMREC_COSINE_MAX_TERMS, rows of d = 64 k floats), coef [n_terms][max_batch][2] as mmrec_cosine_fwd_f32's;
 *   bwd: dX[t][ix[t][b]] += g[0] w[t] / batch[t] (coef.x y - coef.y x) by fp32 atomics (dX[t] NULL: no gradient for that term;
 *   terms may share X / dX).  X, ix, Y, iy, w, batch, dX are HOST arrays of n_terms entries.
 * replaces: the six `1 - cosine_similarity(...).mean()` terms of bm3.py:129-144 (per-term form: mmrec_cosine_fwd/bwd_f32). */
#define MMREC_COSINE_MAX_TERMS 8
size_t mmrec_cosine_multi_workspace_bytes(int32_t n_terms, int32_t max_batch);
int mmrec_cosine_multi_fwd_f32(const float* const* X, const int64_t* const* ix, const float* const* Y, const int64_t* const* iy,
                               const float* w, const int32_t* batch, int32_t n_terms, int32_t d, float* out, float* coef,
                               void* workspace, mmrec_stream_t stream);
int mmrec_cosine_multi_bwd_f32(const float* const* X, const int64_t* const* ix, const float* const* Y, const int64_t* const* iy,
                               const float* w, const int32_t* batch, int32_t n_terms, int32_t d, const float* coef,
                               const float* grad_scalar, float* const* dX, mmrec_stream_t stream);

/* ABI 14 -- F.normalize(x, p=2, dim=1) in one launch each way (lattice.py:165, mmgcn.py:167): Y = X / max(||X_row||, eps),
 * inv[row] = +- 1 / max(||X_row||, eps) (out, for the backward; negative: the clamp was active); bwd: dX = |inv| (G - Y (Y . G))
 * (clamp active: |inv| G).  Rows of d % 4 == 0 floats. */
int mmrec_row_normalize_fwd_f32(const float* X, int64_t n, int32_t d, float eps, float* Y, float* inv, mmrec_stream_t stream);
int mmrec_row_normalize_bwd_f32(const float* Y, const float* G, const float* inv, int64_t n, int32_t d, float* dX,
                                mmrec_stream_t stream);

/* ABI 14 -- the elementwise tail of an MMGCN layer (mmgcn.py:170-173, :176-179, :182-185) in one launch each way:
 *   fwd: out [n, wa + wb] = [ leaky_relu(A [n, wa]) | leaky_relu(B [n, wb]) + R [n, wb] ]   (R may be NULL; wa, wb % 4 == 0)
 *   bwd: dA = dOut[:, :wa] * (A > 0 ? 1 : slope), dB likewise from dOut[:, wa:], dR = dOut[:, wa:] (each may be NULL)
 * replaces: F.leaky_relu x 2, the `+ id_embedding`, torch.cat((h, x_hat), dim=1) and their four backward launches. */
int mmrec_cat_leaky_fwd_f32(const float* A, const float* B, const float* R, int64_t n, int32_t wa, int32_t wb, float slope,
                            float* out, mmrec_stream_t stream);
int mmrec_cat_leaky_bwd_f32(const float* A, const float* B, const float* dOut, int64_t n, int32_t wa, int32_t wb, float slope,
                            float* dA, float* dB, float* dR, mmrec_stream_t stream);


/* In-batch InfoNCE between two views of the same ids (d = 64), logits never materialised:
 *   v1 = normalize(E1[ids]), v2 = normalize(E2[ids])  (F.normalize, eps 1e-12)
 *   loss[0] = mean_i -log( exp(<v1_i,v2_i>/tau) / sum_j exp(<v1_i,v2_j>/tau) )
 * replaces MGCN.InfoNCE -- mgcn.py:224-231 as called at mgcn.py:252-253 (and its autograd).
 * The backward call takes the workspace the forward call filled and accumulates into dE1 / dE2
 * (dense tables, either may be NULL); grad_loss is a device scalar. */
size_t mmrec_infonce_workspace_bytes(int32_t batch);
int mmrec_infonce_fwd_f32(const float* E1, const float* E2, const int64_t* ids, int32_t batch,
                          int32_t d, float tau, float* loss, void* workspace, mmrec_stream_t stream);
int mmrec_infonce_bwd_f32(const int64_t* ids, int32_t batch, int32_t d, float tau,
                          const float* grad_loss, float* dE1, float* dE2, void* workspace,
                          mmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * P3  modal feature projection (fp32 MFMA, exact fp32):  Y[n,64] = X[n,F] W[64,F]^T + b
 * replaces: nn.Linear image_trs / text_trs / item_linear -- freedom.py:205,208  bm3.py:102,104
 *           lattice.py:134,136  vbpr.py:70 ; and autograd's dW = dY^T X, db = sum dY, dX = dY W.
 * F must be a multiple of 4; out features must be 64 (mmrec_linear_bwd_w_f32 also takes out = 64 j:
 * dY [n, out], dW [out, F], db [out]).  `workspace` (split-K partials) size from
 * mmrec_linear_workspace_bytes.  Deterministic (partials are summed in order).

 * Wider layers (MMGCN's 4096 -> 256 MLP and 256 x 256 / 384 x 384 convolution weights, mmgcn.py:46-
 * 60,164-188): forward and dX are mmrec_gemm_nt_f32, dW / db the out = 64 j form above.
 * ---------------------------------------------------------------------------------------------- */
size_t mmrec_linear_workspace_bytes(int32_t n, int32_t F, int32_t out);
int mmrec_linear_fwd_f32(const float* X, const float* W, const float* b, float* Y, int32_t n,
                         int32_t F, int32_t out, void* workspace, mmrec_stream_t stream);
/* ABI 8 -- the same projection on the 16-bit matrix cores with SPLIT operands: x = hi + 2^-11 lo' in fp16, three fp16 MFMA
 * products per 16 k instead of eight fp32 ones (fp32-input MFMA is 1/16 of the 16-bit rate and bounds the fp32 form), fp32
 * accumulators, error <= 2^-21 |x||w| per term -- as accurate against float64 as the fp32 form.
 * The whole fp32 range is served (round 5): rows of X / W outside what fp16 can hold -- |.| >= 65520, inf, NaN (found as a
 * non-finite result), or a row whose largest magnitude is below 2^-10 and not 0 -- are detected ON THE DEVICE and their
 * 128-row blocks recomputed by the fp32 kernel inside the same call (flags in the workspace, a second launch that returns at
 * once for unflagged blocks; no host synchronisation, capture-safe).  Unflagged rows: |err| <= 2^-21 sum |x w| + 2^-25 max|x_row|
 * sum |w_row|.  Arguments, workspace (mmrec_linear_workspace_bytes) and results (to rounding) as mmrec_linear_fwd_f32;
 * F % 32 != 0 is served by it. */
int mmrec_linear_fwd_split_f32(const float* X, const float* W, const float* b, float* Y, int32_t n, int32_t F,
                               int32_t out, void* workspace, mmrec_stream_t stream);
/* ABI 11 -- the projection's BACKWARD with split operands, one call: dW [64, F] = dY^T X, db [64] = column sums of dY (fp32,
 * fixed order), dX [n, F] = dY W  (autograd of nn.Linear: freedom.py:58-62,205,208; bm3.py:51-56; lattice.py:90-92).  dW (with
 * db or without) and dX may each be NULL (not wanted).  inf / NaN give non-finite results where F.linear's backward has them.
 *   dW  both operands as THREE bf16 parts (x = b1 + b2 + b3 exactly to 2^-24; bf16 has fp32's exponent range: no scales, no
 *       guard, no second launch), six products per 16 items in one fp32 accumulator set:
 *       |err| <= 2^-22 sum |dy x| per output + fp32 accumulation, for any magnitudes; entries below 2^-110 are carried to an
 *       absolute 2^-133 (bf16's smallest denormal) instead of a relative 2^-24.
 *       (The first form used two fp16 halves and one power-of-two scale per column of dY behind a range guard: the gradient
 *       columns of a real batch span more than any one scale holds and the guard's fp32 fix-up ran on most training steps.)
 *   dX  two fp16 halves of dY and W, three products, the operands brought into fp16's range by exact power-of-two scales (per
 *       row of dY, in registers; per column of W): |err| <= 2^-21 sum |dy w| per output as long as the entries of a dY ROW / a
 *       W COLUMN lie within 2^28 of that row's / column's maximum; smaller entries carry an absolute error of 2^-36 of the
 *       maximum's power of two (negligible against the sum unless the large entries' partners are exactly zero).  Stated, not
 *       guarded.
 * out == 64 and F % 128 == 0 run these kernels, every other shape is handed to mmrec_linear_bwd_w_f32 / mmrec_linear_bwd_x_f32.
 * A db without a dW is MMREC_ERR_BAD_ARG for every shape, those handed to the fp32 entry points included, before any launch.
 * Deterministic (no float atomics).
 * workspace: mmrec_linear_bwd_split_workspace_bytes (>= mmrec_linear_workspace_bytes). */
size_t mmrec_linear_bwd_split_workspace_bytes(int32_t n, int32_t F, int32_t out);
int mmrec_linear_bwd_split_f32(const float* dY, const float* X, const float* W, float* dW, float* db, float* dX, int32_t n,
                               int32_t F, int32_t out, void* workspace, mmrec_stream_t stream);
/* dW [out, F] = dY^T X, db [out] = column sums of dY (NULL: not wanted); out = 64 j, every 64-column group of dY in one launch.
 * Returns, in this order and before any launch: out <= 0, out % 64 != 0, F <= 0 or F % 4 != 0: MMREC_ERR_UNSUPPORTED; n < 0:
 * MMREC_ERR_BAD_ARG; NULL dW: MMREC_ERR_BAD_ARG; n == 0: dW = 0 (and db = 0 where given) are written, dY / X / workspace may be
 * NULL; n > 0 with a NULL dY / X / workspace: MMREC_ERR_BAD_ARG. */
int mmrec_linear_bwd_w_f32(const float* dY, const float* X, float* dW, float* db, int32_t n,
                           int32_t F, int32_t out, void* workspace, mmrec_stream_t stream);
int mmrec_linear_bwd_x_f32(const float* dY, const float* W, float* dX, int32_t n, int32_t F,
                           int32_t out, mmrec_stream_t stream);
/* ABI 15 -- the projection of LISTED rows of a feature table, straight from the table (freedom.py:203-208, bm3.py:116 with
 * lazy_projection: the batch's pos / neg rows): no [n, F] copy of the rows is written or read.
 *   fwd  Y [n, 64] = T[ids] W^T + b                    split != 0: the split-operand kernel of mmrec_linear_fwd_split_f32 with its
 *                                                      device-side domain guard and fp32 fix-up, 0: the fp32 LDS-DMA kernel
 *   bwd  dW [64, F] = dY^T T[ids], db [64] = column sums of dY, dX [n, F] = dY W: COMPACT, one row per list position (the caller
 *        adds the rows of duplicated ids into the table's gradient).  dW (with db or without) and dX may each be NULL.
 * T [n_table, F] contiguous; ids [n] int64: values in [0, n_table) name a row, duplicates allowed, ANY other value (-1: "no
 * row") reads as a row of zeros -- Y = b there, nothing added to dW -- and is never used as an address.  Row offsets are 64-bit:
 * tables above 4 GiB are served.
 * Served: out == 64 and F % 128 == 0 (MMREC_ERR_UNSUPPORTED otherwise).  The kernels, split plans and summation orders are those
 * of the dense entry points for the same (n, F): every result equals, bit for bit, the dense call on a gathered copy of the rows.
 * Deterministic (no float atomics), no host synchronisation, capture-safe.
 * workspace: mmrec_linear_rows_workspace_bytes. */
size_t mmrec_linear_rows_workspace_bytes(int32_t n, int32_t F, int32_t out);
int mmrec_linear_rows_fwd_f32(const float* T, int64_t n_table, const int64_t* ids, const float* W, const float* b, float* Y,
                              int32_t n, int32_t F, int32_t out, int32_t split, void* workspace, mmrec_stream_t stream);
int mmrec_linear_rows_bwd_f32(const float* dY, const float* T, int64_t n_table, const int64_t* ids, const float* W, float* dW,
                              float* db, float* dX, int32_t n, int32_t F, int32_t out, void* workspace, mmrec_stream_t stream);
/* C[M, :N] = A[M, K] B[N, K]^T (+ bias[N], may be NULL); K % 32 == 0, N <= ldc <= 2 Mi (32-bit byte offsets within a 128-row block).
 * F.linear(x, W, b) is (A, B) = (x, W); its dX is (A, B) = (dY, W^T).
 * Only columns 0 .. N-1 of a row of C are written: columns N .. ldc-1 (ldc > N) are left untouched.
 * Returns, in this order and before any launch: K <= 0, K % 32 != 0, N <= 0, ldc < N or ldc > 2^21: MMREC_ERR_UNSUPPORTED;
 * M < 0: MMREC_ERR_BAD_ARG; M == 0: 0, no launch, nothing written (pointers may be NULL); NULL A / B / C: MMREC_ERR_BAD_ARG.
 * Deterministic (no atomics). */
int mmrec_gemm_nt_f32(const float* A, const float* B, const float* bias, float* C, int32_t M, int32_t N,
                      int32_t K, int32_t ldc, mmrec_stream_t stream);

/* ABI 16 -- per-edge dot products (SDDMM): out[e] = <A[rows[e]], B[cols[e]]>, e < n_edges.
 * replaces: build_sim restricted to the kept pairs -- lattice.py:141,146 (utils/utils.py:134-137, :119-122); GRCN's edge scores
 *           torch.mul(x_i, x_j).sum(dim=-1) -- grcn.py:63; and d vals of the product with learned values, the backward of
 *           torch.mm(self.item_adj, h) -- lattice.py:163 -- with respect to the adjacency's entries.
 * A [n_a, d], B [n_b, d] row-major (B may be A); rows / cols [n_edges] int64 in any order, duplicates allowed; row offsets are
 * 64-bit.  d = 8 / 16 / 32 or a multiple of 64 up to 384 -- what mmrec_spmm_csr_f32 accepts -- anything else:
 * MMREC_ERR_UNSUPPORTED (checked before the pointers).  Null pointers or negative sizes: MMREC_ERR_BAD_ARG; n_edges == 0: 0 and
 * no launch; n_edges > 2^31 - 1: MMREC_ERR_UNSUPPORTED.
 * An edge whose row id is outside [0, n_a) or whose column id is outside [0, n_b) (-1: "no edge") gets out[e] = 0 and adds
 * nothing in the backward; its id is never used as an address.
 * Forward: one group of min(d, 64) / 4 lanes per edge, one float4 of each row per lane and 64 columns, one fma chain per lane
 * (d / 16 terms; 4 for the slices), then a fixed butterfly over the group: the same bits run after run.
 * Backward: dA[rows[e]] += g[e] * B[cols[e]] ; dB[cols[e]] += g[e] * A[rows[e]]  (either may be NULL; dA == dB allowed when
 * A == B: both sums land in the one buffer).  fp32 atomics into caller-zeroed / accumulating buffers, so the order of a row's
 * sum -- its last ulp -- can differ from run to run (callers that need fixed bits run the two sums as mmrec_spmm_csr_f32 over
 * the edge list's CSR forms: hip_ops.edge_dot with a DynGraph).
 * No synchronisation, no allocation, capture-safe, no global state. */
int mmrec_edge_dot_f32(const float* A, int64_t n_a, const float* B, int64_t n_b,
                       const int64_t* rows, const int64_t* cols, int64_t n_edges, int32_t d,
                       float* out, mmrec_stream_t stream);
int mmrec_edge_dot_bwd_f32(const float* g, const float* A, int64_t n_a, const float* B, int64_t n_b,
                           const int64_t* rows, const int64_t* cols, int64_t n_edges, int32_t d,
                           float* dA, float* dB, mmrec_stream_t stream);

/* Segment softmax over the edges that share a node, and its backward -- the step between mmrec_edge_dot_f32 and the product
 * with learned values.  ADDITIVE to ABI 16: three new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: torch_geometric.utils.softmax(alpha, index) -- grcn.py:69 (scatter-max, gathers, exp, scatter-add, divide).
 * Segments are the rows of a CSR rowptr [n_rows + 1] (device, int32).  Entry j of row r, rowptr[r] <= j < rowptr[r + 1], lives
 * at position p = perm ? perm[j] : j of score / out / alpha / g / ds [n_edges]: input and output are in the caller's (COO)
 * order, like mmrec_edge_dot_f32's.  perm [n_edges] int64 (device), NULL = identity; a position outside [0, n_edges) is skipped
 * and never used as an address.
 *   forward   out[p] = exp(s[p] - m_r) / (sum_q exp(s[q] - m_r) + eps),  m_r = max_q s[q] over row r
 *   backward  ds[p]  = alpha[p] * (g[p] - sum_q alpha[q] g[q])  -- reads the forward's result, not the scores; the exact
 *             derivative of the forward with the maximum detached; WRITES ds, does not add into it.
 * Rows of at most mmrec_segment_softmax_group_max() entries: one 16-lane group per row; longer rows: one workgroup per row,
 * taken from long_rows [n_long] (device, int32, ascending) -- exactly the rows longer than that constant, which is what
 * mmrec_spmm_plan_fill writes when called with the constant as its threshold.  The constant is ONE value for the three per-row
 * edge ops: mmrec_edge_attention_group_max() and mmrec_neighbor_max_group_max() return the same number, so one list per CSR
 * serves all of them.  A list that names other rows than those leaves
 * entries of out unwritten (a device list cannot be checked here; hip_ops checks it on the host when it builds it).
 * n_long == 0 (long_rows may be NULL): the 16-lane groups serve every row, whatever its length.
 * No atomics, every sum in an order fixed by the row's length: both directions repeat bit for bit.  Empty rows write nothing.
 * A row that holds a NaN, a +inf or nothing but -inf is NaN in every entry and no other row is affected; a -inf entry next to
 * a finite maximum is exactly 0.  out must not be score, ds must not be alpha or g.
 * Negative sizes: MMREC_ERR_BAD_ARG; n_edges == 0 or n_rows == 0: 0 and no launch (pointers may be NULL); n_edges > 2^31 - 1:
 * MMREC_ERR_UNSUPPORTED; NULL rowptr / score / out (alpha / g / ds): MMREC_ERR_BAD_ARG; n_long > 0 with NULL long_rows:
 * MMREC_ERR_BAD_ARG -- in this order, before any launch.  No synchronisation, no allocation, capture-safe, no global state. */
int32_t mmrec_segment_softmax_group_max(void);
int mmrec_segment_softmax_f32(const int32_t* rowptr, int32_t n_rows, const int64_t* perm, const int32_t* long_rows,
                              int32_t n_long, const float* score, int64_t n_edges, float eps, float* out,
                              mmrec_stream_t stream);
int mmrec_segment_softmax_bwd_f32(const int32_t* rowptr, int32_t n_rows, const int64_t* perm, const int32_t* long_rows,
                                  int32_t n_long, const float* alpha, const float* g, int64_t n_edges, float* ds,
                                  mmrec_stream_t stream);

/* Fused edge attention ("GAT aggregation"): the scores, the softmax over a row's edges and the weighted sum in one pass --
 * mmrec_edge_dot_f32 -> mmrec_segment_softmax_f32 -> mmrec_spmm_csr_f32 with values, with every source row gathered once.
 * ADDITIVE to ABI 16: two new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: the attention layer of the content GCN -- grcn.py:63-72 (x_i . x_j per edge, softmax over the edges of a target,
 *           the weighted sum of the source rows).
 * Rows are the rows of a CSR (rowptr [n_rows + 1], colidx [n_edges], device, int32); slot j of row r lives at position
 * p = perm ? perm[j] : j of alpha [n_edges] (the caller's COO order; perm as for mmrec_segment_softmax_f32).
 *   s_p     = <Q[r], KV[colidx[j]]>                                     Q [n_q, 64], KV [n_kv, 64] fp32 row-major, n_q >= n_rows
 *   alpha_p = exp(s_p - m_r) / (sum_q exp(s_q - m_r) + eps),            m_r = max over the row
 *   Y[r]    = sum_p alpha_p * KV[colidx[j]]                             Y [n_rows, 64]
 * Q == KV is allowed; Y and alpha must not alias an input.  d == 64 only.  Rows of at most mmrec_edge_attention_group_max()
 * entries: one 16-lane group per row with an online (running-maximum) softmax; longer rows: one workgroup per row of long_rows
 * [n_long] (device, int32) -- the rows longer than that constant as mmrec_spmm_plan_fill lists them at that threshold
 * (mmrec_segment_softmax_f32's list).  n_long == 0: the groups serve every row.  A list that names other rows leaves rows of Y
 * unwritten (hip_ops checks it on the host).
 * EVERY row of Y is written (zeros for a row without edges).  A colidx outside [0, n_kv) or a position outside [0, n_edges) is
 * an absent edge: never an address, adds nothing, its alpha is not written.  No atomics: the bits of Y and alpha are a
 * function of the inputs and the row lengths.  A row whose scores hold a NaN, a +inf or nothing but -inf is NaN in every
 * alpha and in Y[r]; no other row is affected; a -inf score next to a finite maximum weighs exactly 0.
 * d != 64: MMREC_ERR_UNSUPPORTED; negative sizes: MMREC_ERR_BAD_ARG; n_rows == 0 or n_edges == 0: 0 and no launch (pointers
 * may be NULL; with rows and no edges Y is NOT written: the caller's zeros); n_edges or n_kv > 2^31 - 1: MMREC_ERR_UNSUPPORTED;
 * n_q < n_rows, a NULL rowptr / colidx / Q / KV / Y / alpha, n_long > 0 with NULL long_rows: MMREC_ERR_BAD_ARG -- in this
 * order, before any launch.  No synchronisation, no allocation, capture-safe, no global state. */
int32_t mmrec_edge_attention_group_max(void);
int mmrec_edge_attention_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                             const int32_t* long_rows, int32_t n_long, const float* Q, int64_t n_q, const float* KV,
                             int64_t n_kv, int32_t d, int64_t n_edges, float eps, float* Y, float* alpha,
                             mmrec_stream_t stream);

/* Backward of mmrec_edge_attention_f32 from its results alpha and Y, every row gathered once.  ADDITIVE to ABI 16: one new
 * symbol, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: autograd through grcn.py:63-72, and the composition mmrec_edge_dot_f32 -> mmrec_segment_softmax_bwd_f32 -> three
 *           mmrec_spmm_csr_f32 with permuted copies of ds and alpha.
 * With row r, slot j at position p, column c = colidx[j] as in the forward:
 *   g_p    = <dY[r], KV[c]> + dAlpha[p]                         dY [n_rows, 64] and dAlpha [n_edges]: one may be NULL, not both
 *   t_r    = <dY[r], Y[r]> + sum_p alpha_p dAlpha[p]            (= sum_p alpha_p g_p: Y is the forward's, needed only with dY)
 *   ds_p   = alpha_p (g_p - t_r)                                ds [n_edges], caller-owned, ALWAYS written, the caller's order
 *   dQ[r]  = sum_p ds_p KV[c]                                   dQ [n_rows, 64]
 *   dKV[c] = dKV_base[c] + sum over the edges of column c of (alpha_p dY[r] + ds_p Q[r])         dKV, dKV_base [n_kv, 64]
 * the exact derivative of the forward as written (maximum detached, eps in the denominator).  dQ or dKV may be NULL, not both.
 * dKV_base may be NULL and may be dQ (Q == KV: dKV is then the whole gradient); it must not be dKV.  Outputs must not alias
 * inputs.  Row pass (ds, dQ): the forward's CSR, perm, long_rows / n_long and access shape; a listed row's 16 partial sums are
 * added in a fixed order.  Column pass (dKV; its arguments and Q are unused when dKV == NULL): the transposed CSR of the same
 * edge list -- rowptr_t [n_kv + 1], rowidx_t [n_edges] (the row of each slot), perm_t (NULL = identity), and long_cols
 * [n_long_t], the columns with more than mmrec_edge_attention_group_max() entries listed as long_rows is; it reads alpha and
 * ds through perm_t.  n_long == 0 / n_long_t == 0: the 16-lane groups serve every row / column.
 * EVERY row of dQ and of dKV is written.  An absent edge -- a column id outside [0, n_kv), a row id outside [0, n_rows) on the
 * transposed side, a position outside [0, n_edges) -- is never an address and adds nothing; where its position is valid its
 * ds is written as 0.  The two sides must name the SAME edges: the forward leaves alpha undefined at the position of an edge
 * that is absent on the row side, and the column pass decides presence from rowidx_t and perm_t alone, so a transposed CSR
 * that still lists such an edge reads that undefined alpha -- dKV is then undefined.  No atomics: the bits of ds, dQ and
 * dKV are a function of the inputs and the row and column lengths.  A row whose alpha is NaN is NaN in its ds, in dQ[r] and
 * in the dKV rows of its own columns, and nowhere else.  A hub is one workgroup in each pass, as in the forward.
 * d != 64: MMREC_ERR_UNSUPPORTED; negative sizes: MMREC_ERR_BAD_ARG; n_rows == 0 or n_edges == 0: 0 and no launch (pointers
 * may be NULL; nothing is written: the caller's zeros); n_edges or n_kv > 2^31 - 1: MMREC_ERR_UNSUPPORTED; n_q < n_rows, a NULL
 * rowptr / colidx / KV / alpha / ds, dY and dAlpha both NULL, dY without Y, dQ and dKV both NULL, dKV with a NULL rowptr_t /
 * rowidx_t / Q or with dKV_base == dKV, a long count > 0 with a NULL list: MMREC_ERR_BAD_ARG -- in this order, before any
 * launch.  No synchronisation, no allocation, capture-safe, no global state. */
int mmrec_edge_attention_bwd_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                                 const int32_t* long_rows, int32_t n_long, const int32_t* rowptr_t, const int32_t* rowidx_t,
                                 const int64_t* perm_t, const int32_t* long_cols, int32_t n_long_t, const float* Q, int64_t n_q,
                                 const float* KV, int64_t n_kv, const float* Y, const float* alpha, const float* dY,
                                 const float* dAlpha, int32_t d, int64_t n_edges, float* ds, float* dQ, float* dKV,
                                 const float* dKV_base, mmrec_stream_t stream);

/* Max over a node's neighbours with the argmax, and its backward: PyG's `aggr='max'` without the [n_edges, 64] message tensor.
 * ADDITIVE to ABI 16: three new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: Base_gcn(aggr='max').propagate -- dualgnn.py:318-345, dragon.py:387-410 (x[src] gathered per edge, scatter-max at
 *           the targets, and autograd's copies of both).
 * Rows are the rows of a CSR (rowptr [n_rows + 1], colidx [n_edges], device, int32); slot j of row r lives at position
 * p = perm ? perm[j] : j of the caller's edge list (perm as for mmrec_segment_softmax_f32).  X [n_x, 64] fp32 row-major.
 *   Y[r][c]   = max over the slots j of row r of X[colidx[j]][c]                     Y [n_rows, 64] fp32
 *   arg[r][c] = the position p of the slot chosen                                    arg [n_rows, 64] int32
 * SELECTION RULE (part of the contract), per (r, c): the chosen slot is the first in CSR order whose value is NaN; without a
 * NaN it is the first in CSR order that attains the maximum under IEEE `>` (-0 and +0 are tied: the first wins).  Y holds the
 * chosen value's bits (the forward is exact).  A row without (present) entries: Y = 0 and arg = -1.  EVERY row of Y and of arg
 * is written.  A colidx outside [0, n_x) or a position outside [0, n_edges) is an absent edge: never an address, never chosen.
 * Rows of at most mmrec_neighbor_max_group_max() entries: one 16-lane group per row; longer rows: one workgroup per row of
 * long_rows [n_long] (device, int32; mmrec_segment_softmax_f32's list); n_long == 0: the groups serve every row.  A list that
 * names other rows leaves rows unwritten (hip_ops checks it on the host).  The result does not depend on the launch shape: partial
 * states are combined by (is NaN, value, CSR slot).  No atomics.  Y and arg must not alias an input.
 * d != 64: MMREC_ERR_UNSUPPORTED; negative sizes: MMREC_ERR_BAD_ARG; n_rows == 0: 0 and no launch; n_edges or n_x > 2^31 - 1:
 * MMREC_ERR_UNSUPPORTED; a NULL rowptr / Y / arg, n_edges > 0 with a NULL colidx / X, n_long > 0 with NULL long_rows:
 * MMREC_ERR_BAD_ARG -- in this order, before any launch (n_edges == 0 with rows: Y = 0 and arg = -1 ARE written).
 *
 * mmrec_neighbor_max_bwd_f32: a pull over the TRANSPOSED CSR of the same edge list -- rowptr_t [n_cols + 1], rowidx_t
 * [n_edges] (the row of each slot), perm_t (NULL = identity), long_cols [n_long_t] listed as long_rows is:
 *   dX[s][c] = dX_base[s][c] + sum of dY[r][c] over the slots jt of column s with arg[r][c] == p,
 *              r = rowidx_t[jt], p = perm_t ? perm_t[jt] : jt                        dX, dX_base [n_cols, 64], dY [n_rows, 64]
 * dX_base may be NULL; it must not be dX.  The comparison is on positions: of duplicate (r, s) edges only the chosen copy
 * contributes.  Terms are added in slot order by the 16-lane group that owns the column; a listed column's 16 partial sums are
 * added after the base in a fixed order: no atomics, the same bits every call.  EVERY row of dX is written.  An r outside
 * [0, n_rows) or a position outside [0, n_edges) is an absent edge: never an address, adds nothing.
 * d != 64: MMREC_ERR_UNSUPPORTED; negative sizes: MMREC_ERR_BAD_ARG; n_cols == 0: 0 and no launch; n_edges or n_rows > 2^31 - 1:
 * MMREC_ERR_UNSUPPORTED; a NULL rowptr_t / dX, dX_base == dX, n_edges > 0 with a NULL rowidx_t / arg / dY, n_long_t > 0 with
 * NULL long_cols: MMREC_ERR_BAD_ARG -- in this order, before any launch.
 * All three: no synchronisation, no allocation, capture-safe, no global state. */
int32_t mmrec_neighbor_max_group_max(void);
int mmrec_neighbor_max_f32(const int32_t* rowptr, int32_t n_rows, const int32_t* colidx, const int64_t* perm,
                           const int32_t* long_rows, int32_t n_long, const float* X, int64_t n_x, int32_t d, int64_t n_edges,
                           float* Y, int32_t* arg, mmrec_stream_t stream);
int mmrec_neighbor_max_bwd_f32(const int32_t* rowptr_t, int32_t n_cols, const int32_t* rowidx_t, const int64_t* perm_t,
                               const int32_t* long_cols, int32_t n_long_t, const int32_t* arg, int64_t n_rows, const float* dY,
                               int32_t d, int64_t n_edges, float* dX, const float* dX_base, mmrec_stream_t stream);

/* Row-wise log-sum-exp of scale * Q K^T against a whole table, with gradients to both operands, never storing the [B, N]
 * scores.  ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: exp(normalize(e[ids]) @ normalize(all).T / tau).sum(1) -- lgmrec.py:157-164 (the batch against every user / item)
 *           and pgl.py:226-231 (two dropout views of the batch, width 128) -- and autograd's copies of that matrix.
 *   lse[i] = log sum_{j<N} exp(scale <Q[i], K[j]>)            Q [B, d], K [N, d] fp32 row-major, d == 64 or 128, lse [B]
 *   dQ[i]  = scale g[i] sum_j p_ij K[j]                       p_ij = exp(scale s_ij - lse[i]),  g [B] = dL / d lse
 *   dK[j]  = scale sum_i g[i] p_ij Q[i]                       dQ [B, d], dK [N, d]: either may be NULL (not computed)
 * Q == K is allowed (the caller adds dQ and dK); outputs must not alias inputs.  Scores are fp32 fma chains in natural k order
 * on the fp32-input MFMA, recomputed in the backward: lse (the caller's) is the only state between the two calls.  Running
 * maximum and rescaled sum per row: logits of any finite magnitude give a finite lse.  Grid: 128-row tiles x column splits of
 * mmrec_score_lse_split_cols(B, N, 0) columns (a function of B and N alone; 0 for an empty K; mode 1 / 2: the columns of K per
 * split of the dQ sweep / the rows of Q per split of the dK sweep, whose tiles are 128 rows of Q / of K); per-split results
 * are combined in split order.  No atomics: two calls on the same inputs give the same bits, forward and gradients.
 * N == 0: lse = -inf and zero gradients; B == 0: nothing to write but dK, which is zeroed.  A non-finite value in row i of Q
 * may make lse[i] non-finite and leaves every other row's lse unchanged.
 * workspace: mmrec_score_lse_workspace_bytes(B, N, d) bytes (16-byte aligned) serve either call: 2 * splits * B floats for the
 * forward; for the backward the per-split partial gradients, at most 4 (B + N) d floats for each operand.
 * d not 64 / 128 or a negative size: MMREC_ERR_BAD_ARG; B or N > 2^30: MMREC_ERR_UNSUPPORTED; a NULL Q / K / lse / g /
 * workspace where it is needed, dQ and dK both NULL: MMREC_ERR_BAD_ARG -- before any launch.  No synchronisation, no
 * allocation, no data-dependent launch shape, capture-safe, no global state. */
int32_t mmrec_score_lse_split_cols(int32_t B, int32_t N, int32_t mode);
size_t mmrec_score_lse_workspace_bytes(int32_t B, int32_t N, int32_t d);
int mmrec_score_lse_f32(const float* Q, const float* K, int32_t B, int32_t N, int32_t d, float scale, float* lse,
                        void* workspace, mmrec_stream_t stream);
int mmrec_score_lse_bwd_f32(const float* Q, const float* K, int32_t B, int32_t N, int32_t d, float scale, const float* lse,
                            const float* g, float* dQ, float* dK, void* workspace, mmrec_stream_t stream);

/* Hypergraph message passing of LGMRec: the Gumbel-softmax hyperedge assignment with its dropout, and the HGNN layer, each with
 * its backward.  ADDITIVE to ABI 16: six new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: F.gumbel_softmax(x, tau, dim=1) and F.dropout of its result, and HGNNLayer's three torch.mm per layer --
 *           lgmrec.py:23-36, 196-216 ([n, H] operands against a 64-wide table) -- and autograd's mirror of all of it.
 * Served: 1 <= H <= 8, d == 64, fp32 row-major.  H outside that range or d != 64: MMREC_ERR_UNSUPPORTED, checked first.
 *
 * mmrec_hyper_assign_fwd_f32: logits, noise [n, H]; keep [n, H] of 0 / 1 floats or NULL; P [n, H]; p_soft [n, H] or NULL
 *   p = softmax((logits + noise) / tau) over the H entries of a row, the row maximum subtracted (finite logits of any spread
 *   give a finite p);  P = keep ? p * keep / keep_rate : p.  The kernel draws nothing: noise and keep are the caller's.
 *   p_soft, where given, receives p: THE STATE THE BACKWARD NEEDS.  Without a mask P is p (pass P to the backward and NULL
 *   here); with a mask P has lost p at the dropped entries, whose logits still get a gradient.  P must not be p_soft.
 * mmrec_hyper_assign_bwd_f32: s = keep ? dP * keep / keep_rate : dP;  dlogits = p * (s - sum_h p_h s_h) / tau.
 *   A row whose mask is all zero has P = 0 and dlogits = 0.  noise and keep get no gradient.
 * Both: one launch, one thread per row.  n < 0: MMREC_ERR_BAD_ARG; n > 2^30: MMREC_ERR_UNSUPPORTED; n == 0: 0, no launch;
 * a NULL logits / noise / P (p_soft / dP / dlogits): MMREC_ERR_BAD_ARG -- in this order, before any launch.
 *
 * mmrec_hyper_layer_fwd_f32: P_i [I, H], P_u [U, H], X_prev [I, 64] -> lat [H, 64], X_out [I, 64], U_out [U, 64]
 *   lat = P_i^T X_prev;  X_out = P_i lat;  U_out = P_u lat.  U_out may be NULL (not wanted: every layer but the last); P_u is
 *   then not read.  Three launches: reduce (one workgroup per mmrec_hyper_rows_per_block(I) consecutive rows: wave w of its
 *   four walks the w-th quarter of the block in order, one column per lane and H fma accumulators; the four added in order),
 *   finish (per hyperedge, wave k of sixteen adds the blocks k, k + 16, ... in order, the sixteen sums added in order) and
 *   expand (out[r] = P[r][0] lat[0], then one fma per further hyperedge).  X_prev is read once, each output written once.
 *   I == 0: lat = 0 and U_out = 0.  Outputs must not alias inputs.
 * mmrec_hyper_layer_bwd_f32: given dU [U, 64] and dX [I, 64], either of which may be NULL (zeros):
 *   dlat = P_i^T dX + P_u^T dU (the same reduce, item blocks then user blocks, and the same finish; kept in the workspace)
 *   dP_i[r][h] = <dX[r], lat[h]> + <X_prev[r], dlat[h]>;   dP_u[r][h] = <dU[r], lat[h]>;   dX_prev = P_i dlat
 *   Any of dP_i / dP_u / dX_prev may be NULL (not computed).  Three launches.
 * Both: NO ATOMICS, every order fixed by the shape alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_hyper_workspace_bytes(I, U, H) bytes (16-byte aligned) serve either call: 512 floats and one H x 64 partial
 * per block of either side; 0 for an unserved H or a negative size.  mmrec_hyper_rows_per_block(n): the rows one workgroup of
 * the reduce walks for a side of n rows (a multiple of 64; 64 up to 131,072 rows; 0 for n < 0).
 * I < 0 or U < 0: MMREC_ERR_BAD_ARG; I or U > 2^30: MMREC_ERR_UNSUPPORTED; a NULL lat / workspace, I > 0 with a NULL P_i /
 * X_prev / X_out (backward: P_i, and X_prev where dP_i is wanted), U > 0 with a NULL P_u where U_out (dU) is given:
 * MMREC_ERR_BAD_ARG -- in this order, before any launch.  No synchronisation, no allocation, no data-dependent launch shape,
 * capture-safe, no global state. */
int32_t mmrec_hyper_rows_per_block(int64_t n);
size_t mmrec_hyper_workspace_bytes(int64_t I, int64_t U, int32_t H);
int mmrec_hyper_assign_fwd_f32(const float* logits, const float* noise, const float* keep, int64_t n, int32_t H, float tau,
                               float keep_rate, float* P, float* p_soft, mmrec_stream_t stream);
int mmrec_hyper_assign_bwd_f32(const float* p_soft, const float* keep, const float* dP, int64_t n, int32_t H, float tau,
                               float keep_rate, float* dlogits, mmrec_stream_t stream);
int mmrec_hyper_layer_fwd_f32(const float* P_i, const float* P_u, const float* X_prev, int64_t I, int64_t U, int32_t H,
                              int32_t d, float* U_out, float* X_out, float* lat, void* workspace, mmrec_stream_t stream);
int mmrec_hyper_layer_bwd_f32(const float* P_i, const float* P_u, const float* X_prev, const float* lat, const float* dU,
                              const float* dX, int64_t I, int64_t U, int32_t H, int32_t d, float* dP_i, float* dP_u,
                              float* dX_prev, void* workspace, mmrec_stream_t stream);

/* The same at 64 hyperedges (Clothing's hyper_num; csrc/hypergraph64.hip).  ADDITIVE to ABI 16: six new symbols, nothing existing
 * changes (mmrec_hyper_* still answer MMREC_ERR_UNSUPPORTED above 8), MMREC_ABI_VERSION stays 16.
 * H = 64 and d = 64 are fixed: every operand is [n, 64] fp32 row-major, lat is [64, 64].  The formulas, the state kept between
 * the assignment's two calls (p), the NULL conventions and the order of the argument checks are those of the family above.
 *
 * mmrec_hyper64_assign_fwd_f32 / _bwd_f32: 16 lanes per row, lane t holding the entries 4 t .. 4 t + 3.  The maximum and the sum
 *   ((e0 + e1) + e2) + e3 of a lane's four, then a butterfly over the 16 lanes at the distances 8, 4, 2, 1; exp is expf, the
 *   quotients are fp32 divisions; the backward's dot product is an fma chain over the lane's four from 0, then the butterfly.
 *   n < 0: MMREC_ERR_BAD_ARG; n > 2^30: MMREC_ERR_UNSUPPORTED; n == 0: 0, no launch; a NULL logits / noise / P, P == p_soft
 *   (p_soft / dP / dlogits): MMREC_ERR_BAD_ARG -- in this order, before any launch.
 * mmrec_hyper64_layer_fwd_f32 / _bwd_f32: three launches each.
 *   reduce    one workgroup per block of R = mmrec_hyper64_rows_per_block(n) consecutive rows of a side, walked as 64-row tiles;
 *             part[block][h][c] = ONE chain acc = fma(P[r][h], V[r][c], acc) from 0 over the block's rows in order (R fmas; rows
 *             past n are zeros).  The backward's dlat = P_i^T dX + P_u^T dU runs the item blocks, then the user blocks, in one
 *             launch; a NULL gradient adds no blocks.
 *   finish    per output float, thread `quarter` of four adds the blocks quarter, quarter + 4, ... in order from 0, then the
 *             four sums are added in order: ceil(blocks / 4) + 3 additions.  A term of lat (dlat) meets at most
 *             R + ceil(blocks / 4) + 3 roundings (dlat: the larger R, both sides' blocks).
 *   row pass  X_out[r][c] (U_out, dX_prev) = one chain of 64 fmas from 0 over h ascending of P[r][h] lat[h][c] (dlat).
 *             dP_i[r][h] = ONE chain of 128 fmas from 0: dX[r][c] lat[h][c] for c ascending, then X_prev[r][c] dlat[h][c] for c
 *             ascending (a NULL dX: the second 64 alone).  dP_u[r][h] = 64 fmas over dU[r][c] lat[h][c] (a NULL dU: zeros).
 *             Items and users in one launch, lat (and dlat) in LDS.
 *   U_out NULL: the user rows are neither computed nor written and P_u is not read.  Any of dP_i / dP_u / dX_prev may be NULL
 *   (not computed).  I == 0: lat = 0 and U_out = 0; a side of no rows launches nothing.  NO ATOMICS, every order a function of
 *   I and U alone: two calls on the same inputs give the same bits.  Outputs must not alias inputs.
 *   I < 0 or U < 0: MMREC_ERR_BAD_ARG; I or U > 2^30: MMREC_ERR_UNSUPPORTED; a NULL lat / workspace, I > 0 with a NULL P_i /
 *   X_prev / X_out (backward: P_i, and X_prev where dP_i is wanted), U > 0 with a NULL P_u where U_out (dU) is given:
 *   MMREC_ERR_BAD_ARG -- in this order, before any launch.
 * mmrec_hyper64_rows_per_block(n): R for a side of n rows: 64 while 256 blocks cover it (n <= 16,384), then
 *   64 ceil(n / 16,384); 0 for n < 0 or n > 2^30.  mmrec_hyper64_workspace_bytes(I, U) = 4 * 4096 * (1 + blocks(I) + blocks(U)) with
 *   blocks(n) = ceil(n / R(n)): dlat and one [64][64] partial per block; serves either layer call, 16-byte aligned; 0 for a
 *   negative count or one above 2^30.  No synchronisation, no allocation, no data-dependent launch shape, capture-safe. */
int32_t mmrec_hyper64_rows_per_block(int64_t n);
size_t mmrec_hyper64_workspace_bytes(int64_t I, int64_t U);
int mmrec_hyper64_assign_fwd_f32(const float* logits, const float* noise, const float* keep, int64_t n, float tau,
                                 float keep_rate, float* P, float* p_soft, mmrec_stream_t stream);
int mmrec_hyper64_assign_bwd_f32(const float* p_soft, const float* keep, const float* dP, int64_t n, float tau, float keep_rate,
                                 float* dlogits, mmrec_stream_t stream);
int mmrec_hyper64_layer_fwd_f32(const float* P_i, const float* P_u, const float* X_prev, int64_t I, int64_t U, float* U_out,
                                float* X_out, float* lat, void* workspace, mmrec_stream_t stream);
int mmrec_hyper64_layer_bwd_f32(const float* P_i, const float* P_u, const float* X_prev, const float* lat, const float* dU,
                                const float* dX, int64_t I, int64_t U, float* dP_i, float* dP_u, float* dX_prev,
                                void* workspace, mmrec_stream_t stream);

/* SMORE's spectrum step: rfft of two [n, 64] tables, three complex filters, three irfft, with its backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: torch.fft.rfft(dim=1, norm='ortho') of the image and text tables, the element-wise products with
 *           view_as_complex of the three [1, 33, 2] weights (image, text, and text_fft * image_fft for the fusion filter) and the
 *           three torch.fft.irfft(n=64) -- smore.py:188-206 -- and autograd's mirror of it.
 * Served: d == 64, n <= 2^30, fp32 row-major; anything else: MMREC_ERR_UNSUPPORTED, checked first.
 *
 * Per row, with x the image and y the text row, (a, b) = rfft(x), (c, e) = rfft(y) as real / imaginary parts of the 33 bins:
 *   p3 = c a - e b, q3 = c b + e a;   filter (p, q) with w = (wr, wi):  P = p wr - q wi, Q = p wi + q wr, out = irfft(P, Q)
 *   out_img = filter((a, b), w_img), out_txt = filter((c, e), w_txt), out_fus = filter((p3, q3), w_fus).
 * Weights are [33][2] interleaved (re, im): the memory of the model's [1, 33, 2] parameter.  The imaginary parts of bins 0 and
 * 32 do not enter a real inverse: those two imaginary weights are NEVER READ (no output bit depends on them) and their
 * gradients are written as exactly 0.0.
 *
 * THE PLAN.  A row's spectrum is packed into 64 floats (re_0 .. re_32, im_1 .. im_31), so every transform is a [rows, 64] x
 * [64, 64] product with F[j][k] = cos(2 pi j k / 64) / 8, F[j][32 + k] = -sin(2 pi j k / 64) / 8 or its transpose; the factor 2
 * of the inverse's bins 1 .. 31 is applied in the filter, exactly.  Twiddles: one table of cos(2 pi j / 64) rounded from
 * float64 with exact 0 and +-1, indexed (j k) & 63, scaled by the power of two 1 / 8.  One workgroup per block of
 * mmrec_spectrum_rows_per_block(n) consecutive rows (a multiple of 64; 64 up to 65,536 rows, at most 1,024 blocks), walked in
 * tiles of 64 rows that stay in LDS.  A product ("stage") is one fma chain of 64 terms from 0 per output, the summed index
 * ascending: 64 roundings, and the matrix entry's own counted as 2: S = 66.  Every filter expression is one multiply and one fma.
 * mmrec_spectrum_fwd_f32: ONE launch; x and y read once, each output written once.  Roundings a term of an output meets:
 *   out_img / out_txt: S + 2 + S = 134;   out_fus: (S + S) + 2 + 2 + S = 202.
 * mmrec_spectrum_bwd_f32: given g_img, g_txt, g_fus [n, 64], each of which may be NULL (zeros; its transform is skipped):
 *   (dP, dQ) = g F scaled as the inverse;  dwr = sum_rows (dP p + dQ q), dwi = sum_rows (-dP q + dQ p);
 *   dp = dP wr + dQ wi, dq = -dP wi + dQ wr;  image: da += dp, db += dq;  text: dc += dp, de += dq;
 *   fusion: da += dp c + dq e, db += -dp e + dq c, dc += dp a + dq b, de += -dp b + dq a;  dx = (da, db) F^T, dy = (dc, de) F^T.
 *   The spectra are RECOMPUTED from x and y: the state between the two calls is x, y and the weights.  Two launches: the main
 *   pass, which leaves one [3][33][2] partial per block in the workspace, and the finish (not launched where no weight gradient
 *   is wanted), in which lane l of a wave adds the blocks l, l + 64, ... in order and a fixed butterfly adds the 64 lanes.
 *   Roundings: dx / dy: 3 S + 4 = 202;  a weight gradient: 134 (image, text) or 202 (fusion) for the term, then
 *   rows_per_block / 64 + 6 in the block and ceil(blocks / 64) + 6 in the finish.
 *   Any of dx, dy, dw_img, dw_txt, dw_fus may be NULL (not computed).  A wanted gradient that no given g reaches is written as
 *   zeros (dw_img with g_img NULL).
 * NO ATOMICS, every order fixed by n alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_spectrum_workspace_bytes(n) bytes (16-byte aligned), 198 floats per block; 0 for n < 0 or n > 2^30; needed
 * only where a weight gradient is wanted.  Outputs must not alias inputs.
 * d != 64 or n > 2^30: MMREC_ERR_UNSUPPORTED; n < 0: MMREC_ERR_BAD_ARG; n == 0: 0, no launch; a NULL x / y / weight / forward
 * output, or a NULL workspace where a weight gradient is wanted: MMREC_ERR_BAD_ARG -- in this order, before any pointer is
 * followed.  No synchronisation, no allocation, no data-dependent launch shape, capture-safe (the first call on a device raises
 * the kernels' LDS limit: make one call before capturing). */
int32_t mmrec_spectrum_rows_per_block(int64_t n);
size_t mmrec_spectrum_workspace_bytes(int64_t n);
int mmrec_spectrum_fwd_f32(const float* x, const float* y, const float* w_img, const float* w_txt, const float* w_fus, int64_t n,
                           int32_t d, float* out_img, float* out_txt, float* out_fus, mmrec_stream_t stream);
int mmrec_spectrum_bwd_f32(const float* x, const float* y, const float* w_img, const float* w_txt, const float* w_fus,
                           const float* g_img, const float* g_txt, const float* g_fus, int64_t n, int32_t d, float* dx, float* dy,
                           float* dw_img, float* dw_txt, float* dw_fus, void* workspace, mmrec_stream_t stream);

/* MGCN's behaviour-aware fuser over [n, 64] tables: modality attention, two preference gates and the mix, with its backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: softmax(cat(query_common(image), query_common(text))), the weighted common part, the two sigmoid gates of the
 *           content, the three-way mean and content + side -- mgcn.py:188-203 -- and autograd's mirror of it.
 * Served: d == 64, n <= 2^30, fp32 row-major; anything else: MMREC_ERR_UNSUPPORTED, checked first.
 *
 * V (image), T (text), C (content) [n, 64];  Wq, Wv, Wt [64][64] as torch's [out][in];  bq, q, bv, bt [64].  Per row:
 *   zV = V Wq^T + bq, hV = tanh(zV), sV = <hV, q>   (zT, hT, sT from T with the same Wq, bq, q)
 *   mx = max(sV, sT), aV = e^(sV - mx) / (e^(sV - mx) + e^(sT - mx)), aT likewise;   m = aV V + aT T
 *   pV = sigmoid(C Wv^T + bv), pT = sigmoid(C Wt^T + bt);   side = (pV (V - m) + pT (T - m) + m) / 3;   out = C + side
 *
 * THE PLAN.  One workgroup per block of mmrec_modal_fusion_rows_per_block(n) consecutive rows (64 ceil(n / 16,384): a multiple
 * of 64, a function of n alone, at most 256 blocks), walked in tiles of 64 rows that stay in LDS with the three matrices.  All
 * arithmetic is fp32; every operation named below is ONE rounding (an fma is one), in this order (where a product feeds only an
 * addition the compiler may contract the two into one fma: a rounding fewer, never one more):
 *   z, u     a chain of 64 fma over the input column k ascending, started at the bias.
 *   tanh     qe = expf(-2 |z|), h = copysign((1 - qe) / (1 + qe), z);   sigmoid: qe = expf(-|z|), p = (z >= 0 ? 1 : qe) / (1 + qe).
 *            The argument of expf is exact and <= 0; h is exactly +-1 and p exactly 1 or 0 once qe underflows to 0: never a NaN.
 *   s        over the columns c = l, l + 16, l + 32, l + 48 (l = 0 .. 15): s = fma(h_c, q_c, s) from 0, then the 16 partial sums
 *            by a butterfly (xor 8, 4, 2, 1): 4 + 4 roundings.
 *   a        eV = expf(sV - mx), eT = expf(sT - mx), den = eV + eT, aV = eV / den, aT = eT / den.
 *   mix      m = fma(aT, T, aV V), xV = V - m, xT = T - m, side = fma(pT, xT, fma(pV, xV, m)) / 3, out = C + side.
 * mmrec_modal_fusion_fwd_f32: ONE launch; V, T, C read once, side and out written once.
 * mmrec_modal_fusion_bwd_f32: given g_side, g_out [n, 64], each of which may be NULL (zeros).  Every intermediate above is
 *   RECOMPUTED from V, T, C and the weights: the state between the two calls is the operands.  Then, per element,
 *   G = g_side + g_out, G3 = G / 3, dm = G3 ((1 - pV) - pT), dpV = G3 xV, dpT = G3 xT;
 *   dot = fma(dm_c, V_c - T_c, dot) over the columns and butterfly of s;   dsV = (aV aT) dot, dsT = -dsV;
 *   dzV = (dsV q) fma(-hV, hV, 1), dzT = (dsT q) fma(-hT, hT, 1);   duV = dpV (pV (1 - pV)), duT = dpT (pT (1 - pT));
 *   dV = a chain of 64 fma of dzV Wq over the output column o ascending, started at fma(aV, dm, G3 pV);   dT alike;
 *   dC = the chain of duV Wv started at g_out (0 if NULL), continued by the chain of duT Wt: 128 fma.
 *   Weight gradients, per block: dWq[o][k] is ONE fma chain from 0 over the block's rows, per tile the 64 terms dzV[r][o] V[r][k]
 *   (r ascending), then the 64 terms dzT[r][o] T[r][k]: 2 rows_per_block roundings;  dWv, dWt alike from duV, duT and C:
 *   rows_per_block.  dbq (terms dzV + dzT), dbv (duV), dbt (duT), dq (fma(dsT, hT, dsV hV)): the rows 4 g .. 4 g + 3 of each
 *   tile are added in order onto one sum per group g of a tile's 16 (rows_per_block / 16 additions), then the 16 groups in order
 *   from 0 (16).  The main pass leaves one partial of 3 (64 64 + 64) + 64 = 12,544 floats per block in the workspace
 *   ([dWq][dWv][dWt][dbq][dbv][dbt][dq]); the finish (a second launch, NOT made where no weight gradient is wanted) adds, per
 *   output, the blocks j, j + 4, j + 8, ... in order from 0 for j = 0 .. 3 and then the four sums in order:
 *   ceil(blocks / 4) + 3 roundings.
 *   Any of the ten outputs may be NULL (not computed).  A wanted gradient with both g NULL is written as zeros.
 * NO ATOMICS, every order fixed by n alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_modal_fusion_workspace_bytes(n) bytes (16-byte aligned), 12,544 floats per block (12.8 MB at most); 0 for
 * n < 0 or n > 2^30; needed only where a weight gradient is wanted.  Outputs must not alias inputs.
 * d != 64 or n > 2^30: MMREC_ERR_UNSUPPORTED; n < 0: MMREC_ERR_BAD_ARG; n == 0: 0, no launch; a NULL operand or forward output,
 * or a NULL workspace where a weight gradient is wanted: MMREC_ERR_BAD_ARG -- in this order, before any pointer is followed.
 * No synchronisation, no allocation, no data-dependent launch shape, capture-safe (the first call on a device raises the
 * kernels' LDS limit: make one call before capturing). */
int32_t mmrec_modal_fusion_rows_per_block(int64_t n);
size_t mmrec_modal_fusion_workspace_bytes(int64_t n);
int mmrec_modal_fusion_fwd_f32(const float* V, const float* T, const float* C, const float* Wq, const float* bq, const float* q,
                               const float* Wv, const float* bv, const float* Wt, const float* bt, int64_t n, int32_t d,
                               float* side, float* out, mmrec_stream_t stream);
int mmrec_modal_fusion_bwd_f32(const float* V, const float* T, const float* C, const float* Wq, const float* bq, const float* q,
                               const float* Wv, const float* bv, const float* Wt, const float* bt, const float* g_side,
                               const float* g_out, int64_t n, int32_t d, float* dV, float* dT, float* dC, float* dWq, float* dbq,
                               float* dq, float* dWv, float* dbv, float* dWt, float* dbt, void* workspace,
                               mmrec_stream_t stream);

/* MVGAE's posterior tail over [n, 64] tables: two products of experts, four reparametrisations, four KL terms and the
 * evaluation table, with its backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: product_of_experts twice, reparametrize four times, kl_loss four times and sigmoid(pd_mu) -- mvgae.py, forward and
 *           calculate_loss -- and autograd's mirror of them: about 140 element-wise launches forward.
 *
 * mu_v, lv_v, mu_t, lv_t, mu_c, lv_c [n, 64]: the image, text and collaborative encoders' means and log-variances.  E_p, E_v,
 * E_t, E_c [n, 64]: the noise of the four reparametrisations, ALL given or ALL NULL (NULL: Z[k] = mu_k, evaluation mode).
 * eps = 1e-8f; it, 0.1f and 0.05f below are the fp32 constants.  Per element,
 *   PoE((mu_a, l_a), (mu_b, l_b)):  T_x = 1 / (exp(l_x) + eps),  S = T_a + T_b,  var = 1 / S,  m = (mu_a T_a + mu_b T_b) var,
 *                                   l = log(var)
 *   (m1, l1) = PoE(v, t);   (mu_p, l_p) = PoE((m1, l1), c)        l1 enters stage 2 as it is: NOT clamped, as in the reference
 *   for k in (p, v, t, c):  lh_k = min(l_k, 10),  Z[k] = mu_k + 0.1 E_k exp(0.5 lh_k)            Z [4, n, 64], order p, v, t, c
 *                           kl[k] = -0.5 / n  sum over rows and columns of (1 + lh_k - mu_k^2 - exp(lh_k))          kl [4]
 *   score = sigmoid(mu_p)                                                                          [n, 64]
 * SUPPORTED DOMAIN: finite inputs with |lv| <= 30.  Over it every intermediate is a normal fp32 number (exp(l) in 9e-14 .. 1.1e13,
 * T in 9e-14 .. 1e8, T^2 <= 1e16, S in 1.8e-13 .. 2e8) and every output and gradient is finite.  Outside it the kernels do not
 * fault (no address depends on the data), and nothing more is promised.
 *
 * THE PLAN.  A 16-lane group per row, one float4 per lane and table.  One 256-thread workgroup per block of
 * R = mmrec_posterior_fusion_rows_per_block(n) = 16 ceil(n / 16,384) consecutive rows (a multiple of 16, a function of n alone, at
 * most 1,024 blocks), walked in R / 16 passes of 16 rows: group g of pass p has the row  block R + 16 p + g.  All arithmetic is
 * fp32; every operation named below is ONE rounding (an fma is one), in this order (where a product feeds only an addition the
 * compiler may contract the two into one fma: a rounding fewer, never one more):
 *   expert   E = expf(l), T = 1 / (E + eps)                          (stage 2's first expert: E = expf(l1), l1 the logf below)
 *   PoE      S = T_a + T_b, var = 1 / S, m = fma(mu_b, T_b, mu_a T_a) var, l = logf(var)
 *   tail     lh = fminf(l, 10), sd = expf(0.5 lh), el = expf(lh), Z = fma(0.1 E_k, sd, mu);  noise NULL: Z = mu, a copy of the bits
 *   KL term  t = fma(-mu, mu, 1 + lh) - el.  A lane adds its four columns in order, ((t_0 + t_1) + t_2) + t_3: 3 additions; the 16
 *            lanes of the row by a butterfly (xor 8, 4, 2, 1): 4; the group adds its rows pass after pass onto one sum from 0:
 *            R / 16; the 16 groups are added in order from 0: 16.  One partial per block and k: the workspace is [blocks][4].
 *   finish   a second launch of ONE workgroup, wave k for kl[k]: lane j adds the blocks j, j + 64, ... in order from 0
 *            (ceil(blocks / 64) additions), the 64 lanes by a butterfly (xor 32, 16, 8, 4, 2, 1): 6;
 *            kl[k] = (-0.5 inv_n) sum, inv_n = 1 / (float)n rounded once on the host.
 *            In all a term meets 3 + 4 + R / 16 + 16 + ceil(blocks / 64) + 6 additions.
 *   sigmoid  q = expf(-|z|), score = (z >= 0 ? 1 : q) / (1 + q): the argument of expf is exact and <= 0; exactly 1 or 0 once q
 *            underflows to 0: never a NaN.
 * mmrec_posterior_fusion_fwd_f32: the main launch and the finish; the ten tables read once, Z and score written once.
 * mmrec_posterior_fusion_bwd_f32: ONE launch, given gZ [4, n, 64] (NULL: zeros) and g_kl [4] ON THE DEVICE (NULL: zeros; never
 *   read by the host).  Every intermediate above is RECOMPUTED from the ten inputs: the state between the two calls is the inputs.
 *   Per element, with ck = g_kl[k] inv_n and gz = gZ[k]:
 *   up_k     gm_k = fma(ck, mu_k, gz);   gl_k = l_k <= 10 ? fma(gz, (0.05 E_k) sd_k, -((0.5 ck) (1 - el_k))) : 0
 *            (l_k == 10 passes the gradient, as at::clamp's backward does; above 10 it is exactly 0; noise NULL: E_k = 0)
 *   PoE backward of (gm, gl), the gradients of (m, l), into expert a (b alike):   w_a = ((T_a T_a) E_a) var,
 *            d mu_a = (gm T_a) var,   d l_a = -(w_a fma(gm, mu_a - m, -gl))
 *   stage 2 from up_p gives (g m1, g l1) and c's share; stage 1 from (g m1, g l1) gives v's and t's shares;
 *   d_mu_k = share + gm_k,  d_lv_k = share + gl_k  for k in (v, t, c).
 *   Any of the six outputs may be NULL (not computed); all six NULL: 0, no launch.  A wanted gradient with gZ and g_kl both NULL
 *   is written as zeros.
 * NO ATOMICS, every order fixed by n alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_posterior_fusion_workspace_bytes(n) = 16 blocks bytes (16 KB at most; 0 for n < 0 or n > 2^30), needed by the
 * forward only.  Outputs must not alias inputs.
 * d != 64, n < 0 or n > 2^30: MMREC_ERR_BAD_ARG; n == 0: 0, no launch, nothing written; a NULL input, some but not all of the
 * four noise pointers, a NULL Z, score, kl or workspace in the forward: MMREC_ERR_BAD_ARG -- in this order, before any pointer
 * is followed.  No synchronisation, no allocation, no data-dependent launch shape, capture-safe. */
int32_t mmrec_posterior_fusion_rows_per_block(int64_t n);
size_t mmrec_posterior_fusion_workspace_bytes(int64_t n);
int mmrec_posterior_fusion_fwd_f32(const float* mu_v, const float* lv_v, const float* mu_t, const float* lv_t, const float* mu_c,
                                   const float* lv_c, const float* E_p, const float* E_v, const float* E_t, const float* E_c,
                                   int64_t n, int32_t d, float* Z, float* score, float* kl, void* workspace,
                                   mmrec_stream_t stream);
int mmrec_posterior_fusion_bwd_f32(const float* mu_v, const float* lv_v, const float* mu_t, const float* lv_t, const float* mu_c,
                                   const float* lv_c, const float* E_p, const float* E_v, const float* E_t, const float* E_c,
                                   const float* gZ, const float* g_kl, int64_t n, int32_t d, float* d_mu_v, float* d_lv_v,
                                   float* d_mu_t, float* d_lv_t, float* d_mu_c, float* d_lv_c, mmrec_stream_t stream);

/* MVGAE's encoder heads over [n, 64] tables: H graph-convolution heads (mean, log-variance) that share ONE aggregated table, each
 * with its output Linear and its skip Linear, with the backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: g_layer_k(leaky(conv_embed_k(x, graph))) + leaky(linear_layer_k(x)) for k = 4, 5 -- mvgae.py, the end of GCN.forward
 *           -- and autograd's mirror of it, given AX = spmm(graph, x): the aggregation is linear, spmm(graph, x W) = AX W.
 * Served: d == 64, 1 <= H <= 4, n <= 2^30, fp32 row-major; anything else: MMREC_ERR_UNSUPPORTED, checked first.
 *
 * AX, X [n, 64];  W [H][64][64] as [in][out] (BaseModel.weight);  G, L [H][64][64] as torch's [out][in];  b, bg, bl [H][64];
 * scale [H][n][64], the dropout mask already divided by the keep rate, or NULL (no dropout);  out [H][n][64].  eps = 1e-12f.
 * Per head h and row, leaky(z) = z > 0 ? z : slope z:
 *   a = AX W_h + b_h,  nrm = max(||a||_2, eps),  u = a / nrm,  d = u scale_h,  hh = leaky(d)
 *   p = X L_h^T + bl_h,                                                        out_h = hh G_h^T + bg_h + leaky(p)
 *
 * THE PLAN.  One workgroup per block of mmrec_encoder_heads_rows_per_block(n) consecutive rows (64 ceil(n / 16,384): a multiple
 * of 64, a function of n alone, at most 256 blocks), walked in tiles of 64 rows.  The HEAD LOOP IS OUTERMOST inside the
 * workgroup: head h's three matrices are staged in LDS, the block's tiles are walked, then head h + 1.  All arithmetic is fp32;
 * every operation named below is ONE rounding (an fma is one; sqrtf and / are correctly rounded), in this order (where a product
 * feeds only an addition the compiler may contract the two into one fma: a rounding fewer, never one more):
 *   a, p     a chain of 64 fma over the input column k ascending, started at the bias (b_h, bl_h).
 *   norm     over the columns c = 4 l, 4 l + 1, 4 l + 2, 4 l + 3 (l = 0 .. 15): ss = fma(a_c, a_c, ss) from 0, then the 16 partial
 *            sums by a butterfly (xor 8, 4, 2, 1): 4 + 4 roundings;  raw = sqrtf(ss), nrm = fmaxf(raw, eps), u = a / nrm,
 *            d = u * scale (scale NULL: d = u, no rounding),  hh = d > 0 ? d : slope * d.
 *   out      a chain of 64 fma over hh's column ascending, started at bg_h; then lp = p > 0 ? p : slope * p and ONE addition
 *            out = chain + lp.
 * mmrec_encoder_heads_fwd_f32: ONE launch; AX and X read once per head, out written once.
 * mmrec_encoder_heads_bwd_f32: given g [H][n][64].  Every intermediate above is RECOMPUTED from the operands: the state between
 *   the two calls is the operands and scale.  Then, per head and element,
 *   dhh = a chain of 64 fma of g G_h over the output column o ascending, from 0;
 *   du = (dhh * (d > 0 ? 1 : slope)) * scale  (scale NULL: the first product alone; d == 0 takes slope, as torch does; a dropped
 *        entry, scale == 0, has du = 0 exactly whatever its sign);
 *   dot = fma(u_c, du_c, dot) over the columns and butterfly of ss;
 *   da = fma(-u, dot, du) / nrm  where raw >= eps;   da = du / nrm = du / eps  where raw < eps (the clamp holds the denominator
 *        constant, as F.normalize's backward does);                              dp = g * (p > 0 ? 1 : slope);
 *   dAX = ONE chain of 64 H fma from 0: head 0's 64 terms da[o] W_0[k][o], o ascending, then head 1's, ...  (each head's
 *        workgroup pass stores the rows and the next pass, the same thread, continues from the stored value);
 *   dX  = ONE chain of 64 H fma from 0 alike, of the terms dp[o] L_h[o][k].
 *   Weight gradients, per block and head: dW_h[k][o] is ONE fma chain from 0 over the block's rows r ascending of AX[r][k] da[r][o]:
 *   rows_per_block roundings;  dG_h[o][k] alike of g[r][o] hh[r][k];  dL_h[o][k] alike of dp[r][o] X[r][k].  db_h (terms da),
 *   dbg_h (g), dbl_h (dp): the rows 4 q .. 4 q + 3 of each tile are added in order onto one sum per group q of a tile's 16, from 0
 *   (rows_per_block / 16 additions), then the 16 groups in order from 0 (16).  The main pass leaves one partial of
 *   3 (64 64 + 64) = 12,480 floats per block and head in the workspace ([block][head][dW | dG | dL | db | dbg | dbl]); the finish
 *   (a second launch, NOT made where no weight gradient is wanted) adds, per output, the blocks j, j + 4, j + 8, ... in order
 *   from 0 for j = 0 .. 3 and then the four sums in order: ceil(blocks / 4) + 3 roundings.
 *   Rows past n are zeros in every tile (g too): they add exact zeros to every sum and are never stored; their scale is not read.
 *   Any of the eight outputs may be NULL (not computed; the three weight gradient chains run if any of the six is wanted); all
 *   eight NULL: 0, no launch.
 * NO ATOMICS, every order fixed by n and H alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_encoder_heads_workspace_bytes(n, H) bytes (16-byte aligned), 12,480 H floats per block (51.2 MB at most); 0
 * for n < 0, n > 2^30 or H outside 1 .. 4; needed only where a weight gradient is wanted.  Outputs must not alias inputs.
 * d != 64, H outside 1 .. 4 or n > 2^30: MMREC_ERR_UNSUPPORTED; n < 0: MMREC_ERR_BAD_ARG; n == 0: 0, no launch, nothing touched;
 * a NULL operand other than scale, a NULL out or g, or a NULL workspace where a weight gradient is wanted: MMREC_ERR_BAD_ARG --
 * in this order, before any pointer is followed.  No synchronisation, no allocation, no data-dependent launch shape or address,
 * capture-safe (the first call on a device raises the kernels' LDS limit: make one call before capturing). */
int32_t mmrec_encoder_heads_rows_per_block(int64_t n);
size_t mmrec_encoder_heads_workspace_bytes(int64_t n, int32_t H);
int mmrec_encoder_heads_fwd_f32(const float* AX, const float* X, const float* W, const float* b, const float* G, const float* bg,
                                const float* L, const float* bl, const float* scale, int64_t n, int32_t d, int32_t H, float slope,
                                float* out, mmrec_stream_t stream);
int mmrec_encoder_heads_bwd_f32(const float* AX, const float* X, const float* W, const float* b, const float* G, const float* bg,
                                const float* L, const float* bl, const float* scale, const float* g, int64_t n, int32_t d,
                                int32_t H, float slope, float* dAX, float* dX, float* dW, float* db, float* dG, float* dbg,
                                float* dL, float* dbl, void* workspace, mmrec_stream_t stream);

/* MMGCN's 64-wide layer over [n, 64] tables: the graph convolution, the skip Linear with the id embedding and the 128 -> 64 Linear
 * over their concatenation, with the backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: h = leaky(conv_embed_k(x, graph)), x_hat = leaky(linear_layer_k(x)) + id_embedding,
 *           x = leaky(g_layer_k(cat(h, x_hat))) for k = 2, 3 -- mmgcn.py, GCN.forward -- and autograd's mirror of it, given
 *           AX = spmm(graph, x): the aggregation is linear, spmm(graph, x Wc) = AX Wc.
 * Served: d == 64, slope > 0, n <= 2^30, fp32 row-major; anything else: MMREC_ERR_UNSUPPORTED, checked first.
 *
 * AX, X [n, 64];  R [n, 64] (the id embedding's rows) or NULL (zeros);  Wc [64][64] as [in][out] (BaseModel.weight);  Wl [64][64]
 * and Wg [64][128] as torch's [out][in], Wg = [Gh | Gx] with Gh = Wg[:, :64] and Gx = Wg[:, 64:];  bl, bg [64];  out [n, 64].
 * Per row, leaky(z) = z > 0 ? z : slope z:
 *   a = AX Wc,  h = leaky(a);    p = X Wl^T + bl,  xh = leaky(p) + R;    q = h Gh^T + xh Gx^T + bg;    out = leaky(q)
 *
 * THE PLAN.  One workgroup per block of mmrec_gcn_layer_rows_per_block(n) consecutive rows (64 ceil(n / 16,384): a multiple of 64,
 * a function of n alone, at most 256 blocks), walked in tiles of 64 rows.  All arithmetic is fp32; every operation named below is
 * ONE rounding (an fma is one), in this order (where a product feeds only an addition the compiler may contract the two into one
 * fma: a rounding fewer, never one more):
 *   a        a chain of 64 fma over the input column k ascending, started at 0;   h = a > 0 ? a : slope * a.
 *   p        a chain of 64 fma over the input column k ascending, started at bl;  xh = (p > 0 ? p : slope * p) + R: ONE addition
 *            (R NULL: none).
 *   q        ONE chain of 128 fma started at bg: the 64 terms h[k] Gh[c][k], k ascending, then the 64 terms xh[k] Gx[c][k],
 *            k ascending;  out = q > 0 ? q : slope * q.
 * mmrec_gcn_layer_fwd_f32: ONE launch; AX, X and R read once, out written once.
 * mmrec_gcn_layer_bwd_f32: given g [n][64] and the forward's out.  a, h, p, xh are RECOMPUTED as above: the state between the two
 *   calls is the operands and out.  Then, per element,
 *   dq  = g * (out > 0 ? 1 : slope)   (the sign of out is the sign of q, since slope > 0; out == 0 takes slope, as torch does);
 *   dh  = a chain of 64 fma of dq Gh over the output column c ascending, from 0;   da = dh * (a > 0 ? 1 : slope);
 *   dxh = a chain of 64 fma of dq Gx over the output column c ascending, from 0;   dp = dxh * (p > 0 ? 1 : slope);   dR = dxh;
 *   dAX = a chain of 64 fma from 0 of the terms da[o] Wc[k][o], o ascending;   dX = alike of the terms dp[o] Wl[o][k].
 *   Weight gradients, per block: dWc[k][o] is ONE fma chain from 0 over the block's rows r ascending of AX[r][k] da[r][o]:
 *   rows_per_block roundings;  dWl[o][k] alike of dp[r][o] X[r][k];  dWg[c][k] alike of dq[r][c] h[r][k] and dWg[c][64 + k] of
 *   dq[r][c] xh[r][k].  dbg (terms dq), dbl (dp): the rows 4 j .. 4 j + 3 of each tile are added in order onto one sum per group
 *   j of a tile's 16, from 0 (rows_per_block / 16 additions), then the 16 groups in order from 0 (16).  The main pass leaves one
 *   partial of 4 (64 64) + 2 (64) = 16,512 floats per block in the workspace ([block][dWc | dGh | dWl | dGx | dbg | dbl]); the
 *   finish (a second launch, NOT made where no weight gradient is wanted) adds, per output, the blocks j, j + 4, j + 8, ... in
 *   order from 0 for j = 0 .. 3 and then the four sums in order: ceil(blocks / 4) + 3 roundings.
 *   Rows past n are zeros in every tile of AX, X, g and out: they add exact zeros to every sum and are never stored; their R is
 *   not read.
 *   Any of the eight outputs may be NULL (not computed; the four weight gradient chains run if any of the five is wanted); all
 *   eight NULL: 0, no launch.
 * NO ATOMICS, every order fixed by n alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_gcn_layer_workspace_bytes(n) bytes (16-byte aligned), 16,512 floats per block (16.9 MB at most); 0 for n < 0
 * or n > 2^30; needed only where a weight gradient is wanted.  Outputs must not alias inputs.
 * d != 64, slope <= 0 (or NaN) or n > 2^30: MMREC_ERR_UNSUPPORTED; n < 0: MMREC_ERR_BAD_ARG; n == 0: 0, no launch, nothing
 * touched; a NULL operand other than R, a NULL out or g, or a NULL workspace where a weight gradient is wanted:
 * MMREC_ERR_BAD_ARG -- in this order, before any pointer is followed.  No synchronisation, no allocation, no data-dependent
 * launch shape or address, capture-safe (the first call on a device raises the kernels' LDS limit: make one call before
 * capturing). */
int32_t mmrec_gcn_layer_rows_per_block(int64_t n);
size_t mmrec_gcn_layer_workspace_bytes(int64_t n);
int mmrec_gcn_layer_fwd_f32(const float* AX, const float* X, const float* R, const float* Wc, const float* Wl, const float* bl,
                            const float* Wg, const float* bg, int64_t n, int32_t d, float slope, float* out, mmrec_stream_t stream);
int mmrec_gcn_layer_bwd_f32(const float* AX, const float* X, const float* R, const float* Wc, const float* Wl, const float* bl,
                            const float* Wg, const float* bg, const float* out, const float* g, int64_t n, int32_t d, float slope,
                            float* dAX, float* dX, float* dR, float* dWc, float* dWl, float* dbl, float* dWg, float* dbg,
                            void* workspace, mmrec_stream_t stream);

/* Top-k of a mix of three row softmaxes against three whole tables, never storing a [B, N] block: DAMRS's pseudo-labels.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: topk(p_a + p_b + 2 p_m, 10) with p = softmax(normalize(h[ids]) @ normalize(h).T, dim=1) for each of three
 *           modalities -- damrs.py:141-180 -- and the nine [b, I] blocks behind it.
 *   c_m[r, j] = <T_m[ids[r]], T_m[j]>                         T_0, T_1, T_2 [N, 64] fp32 row-major; ids [B] int64, or NULL:
 *   S_t[r, j] = sum_m W[t][m] exp(c_m[r, j] - lse[m][r])      rows 0 .. B-1; lse [3][B] (the caller's: mmrec_score_lse_f32 of
 *   list t of row r = the k columns j with the largest S_t    T_m[ids] against T_m at scale 1); W [3][3] on the device
 * in score order, descending, ties by the lower column; out_idx [3][B][k] int32, out_val [3][B][k] (the scores; may be NULL).
 * Scores are the fp32 fma chains of the fp32-input MFMA in natural k order, expf, and fma(W[t][2], p_2, fma(W[t][1], p_1,
 * W[t][0] p_0)) -- the same roundings for every column, so bit-identical table rows score the same bits and tie by column.
 * An id outside [0, N) is never used as an address: its three lists are -1 (values -inf).  A NaN score is never listed.
 * Grid: 128-row tiles x column splits of mmrec_tri_topk_split_cols(B, N) columns (a function of B and N alone, at most 32
 * splits; 0 for an empty table or a size above 2^30); every split keeps exact sorted lists and a finish kernel ranks their entries.  No atomics:
 * two calls on the same inputs give the same bits.  workspace: mmrec_tri_topk_workspace_bytes(B, N, k) bytes, 16-byte aligned.
 * k outside 1 .. 16, N < k, a negative size, a NULL table or lse: MMREC_ERR_BAD_ARG; B or N > 2^30: MMREC_ERR_UNSUPPORTED;
 * B == 0: 0, no launch, nothing touched; a NULL W / out_idx / workspace: MMREC_ERR_BAD_ARG -- in this order, before any launch.
 * mmrec_list_exclude_i32: out[r] [k] = the first k entries of cand[r] [kc] that do not occur in excl[r] [ke], in cand's order
 * (R rows, one thread each).  kc - ke < k, k < 1 or a negative size: MMREC_ERR_BAD_ARG; R == 0: 0, no launch; a NULL cand / out
 * / excl (with ke > 0): MMREC_ERR_BAD_ARG.
 * All: no synchronisation, no allocation, no data-dependent launch shape, capture-safe, no global state. */
int32_t mmrec_tri_topk_split_cols(int32_t B, int32_t N);
size_t mmrec_tri_topk_workspace_bytes(int32_t B, int32_t N, int32_t k);
int mmrec_tri_topk_f32(const float* T0, const float* T1, const float* T2, int32_t N, const int64_t* ids, int32_t B,
                       const float* lse, const float* W, int32_t k, int32_t* out_idx, float* out_val, void* workspace,
                       mmrec_stream_t stream);
int mmrec_list_exclude_i32(const int32_t* cand, const int32_t* excl, int32_t R, int32_t kc, int32_t ke, int32_t k, int32_t* out,
                           mmrec_stream_t stream);

/* MVGAE's reconstruction term: every batch user against the HARDEST of the batch's negatives, for L latents over the same rows,
 * never storing the sigmoid of a table, a gathered block or the [B, B] scores; with its backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: recon_loss / dot_product_decode_neg -- mvgae.py:73-85,164-170 -- four times a step, and autograd's mirror of it.
 *
 * Z [L, N, 64] fp32 row-major, 1 <= L <= 8, 1 <= N <= 2^30; users, pos, neg [B] int64 row ids into every Z[l], 1 <= B <= 65,536.
 * With S = sigmoid(Z[l]) (squash != 0; the sigmoid of mmrec_posterior_fusion_fwd_f32: q = expf(-|z|), (z >= 0 ? 1 : q) / (1 + q))
 * or S = Z[l] (squash == 0), u_b = S[users[b]], p_b = S[pos[b]], n_j = S[neg[j]]:
 *   dp_b = <u_b, p_b>,  a_b = sigmoid(dp_b)
 *   h_b  = max_j <u_b, n_j> over the CANDIDATES j: the positions j < B with neg[j] in [0, N)
 *   arg_b = the LOWEST candidate position that attains h_b                                            arg [L, B] int32
 *   x_b = a_b - sigmoid(h_b),  term_b = softplus(-x_b) / ln 2 = -log2(sigmoid(x_b)),  loss[l] = sum_b term_b         loss [L]
 *   c1_b = dterm / d dp = -(sg (a (1 - a))),  c2_b = dterm / dh = sg (sh (1 - sh)),  sg = sigmoid(-x_b) / ln 2, sh = sigmoid(h_b)
 *                                                                                      coef [L, B, 2] = (c1, c2)
 *   su [L, B, 64] = u_b, the squashed user rows (zeros for a sample that does not contribute), kept for the backward
 * AN ID OUTSIDE [0, N) IS NEVER AN ADDRESS.  A sample b with users[b] or pos[b] out of range, or without any candidate, does not
 * contribute: term 0, arg -1, c1 = c2 = 0.  A negative out of range is no candidate for anybody.
 *
 * THE PLAN.  mmrec_hardest_neg_fwd_f32 is three launches.
 *   sweep    grid (ceil(B / 128) own tiles) x (splits of the negatives) x L; a split walks mmrec_hardest_neg_split_cols(B, L)
 *            negative positions (a multiple of 64, a function of B and L alone: ceil(B / 64) tiles over at most 16 splits, about
 *            ceil(512 / L) workgroups a latent).  Scores are the fp32 fma chains of the fp32-input MFMA in natural k order,
 *            score(b, j) = fma(n_j[63], u_b[63], ... fma(n_j[1], u_b[1], n_j[0] u_b[0])) -- the same roundings at every position,
 *            so equal rows score equal bits.  Selection compares (score, then the lower position) in every lane, between the two
 *            lanes of a user and between splits: it depends on no accumulator order, tile or split.  A tile row that is no
 *            candidate is excluded by a mask, never given a score of its own.  One (max, arg) per (split, l, b).
 *   terms    a thread per (l, b): the splits in order from 0, dp as ONE fma chain from 0 over k = 0 .. 63 of u[k] p[k], then
 *            (one rounding each, expf / log1pf the library's) a = sigmoid(dp), sh = sigmoid(h), x = a - sh,
 *            term = (fmaxf(-x, 0) + log1pf(expf(-|x|))) (1 / ln 2), sg = sigmoid(-x) (1 / ln 2), c1 = -(sg (a (1 - a))),
 *            c2 = sg (sh (1 - sh)); arg, coef and su are written, the term goes to the workspace.
 *   loss     ONE workgroup of 1,024 threads per latent: thread t adds the terms of the samples t, t + 1024, ... in order from 0
 *            (ceil(B / 1024) additions), the 64 lanes of a wave by a butterfly (xor 32, 16, 8, 4, 2, 1): 6, the 16 waves in
 *            order from 0: 16.
 * mmrec_hardest_neg_bwd_f32: ONE launch, given arg, coef and su of the forward and g [L] ON THE DEVICE (never read by the host),
 *   writes the SLOT gradients G [L, 3 B, 64], slots in the order users, pos, neg; a 16-lane group per user or pos slot, a WAVE
 *   per neg slot (the hardest negative of a batch is the same for most of its users: one slot's chain can be B long, and its
 *   owner reads the kept rows su 16 at a time); w1_b = g[l] c1_b, w2_b = g[l] c2_b:
 *     user slot b   t = fma(w2_b, n_arg_b, w1_b p_b)
 *     pos slot b    t = w1_b u_b
 *     neg slot j    t = the fma chain from 0, over the samples b with arg_b == j in ASCENDING b, of fma(w2_b, u_b, t)
 *   G = t (s (1 - s)) with s the slot's own squashed row (squash == 0: G = t).  A slot whose sample does not contribute, or whose
 *   own id is out of range, is zeros.  The caller adds G[l] into dZ[l] at cat(users, pos, neg) with
 *   mmrec_scatter_add_rows_sorted_f32 (one stable sort for all latents).  G NULL: 0, no launch.
 * NO FLOAT ATOMICS, every order fixed by (B, L) alone: two calls on the same inputs give the same bits.
 * workspace: mmrec_hardest_neg_workspace_bytes(B, L) = 4 (2 splits + 1) L B bytes (0 outside the served range), the forward's only.
 * B == 0 CONTRACT: 0 is returned before any pointer is looked at, nothing is launched and NOTHING IS WRITTEN -- loss keeps the
 * caller's bytes (a caller that wants the empty sum writes its own zeros).
 * d != 64, L outside 1 .. 8, B outside 0 .. 65,536, N outside 1 .. 2^30: MMREC_ERR_BAD_ARG; B == 0: 0; a NULL Z / users / pos / neg,
 * a NULL loss / arg / coef / su / workspace (forward), a NULL arg / coef / su / g with a G (backward): MMREC_ERR_BAD_ARG -- in this order,
 * before any pointer is followed.  No synchronisation, no allocation, no data-dependent address or launch shape, capture-safe. */
int32_t mmrec_hardest_neg_split_cols(int32_t B, int32_t L);
size_t mmrec_hardest_neg_workspace_bytes(int32_t B, int32_t L);
int mmrec_hardest_neg_fwd_f32(const float* Z, int64_t N, int32_t L, int32_t d, const int64_t* users, const int64_t* pos,
                              const int64_t* neg, int32_t B, int32_t squash, float* loss, int32_t* arg, float* coef, float* su,
                              void* workspace, mmrec_stream_t stream);
int mmrec_hardest_neg_bwd_f32(const float* Z, int64_t N, int32_t L, int32_t d, const int64_t* users, const int64_t* pos,
                              const int64_t* neg, int32_t B, int32_t squash, const int32_t* arg, const float* coef,
                              const float* su, const float* g, float* G, mmrec_stream_t stream);

/* DAMRS's symmetric KL term between two views of the user-item probabilities, never storing an [m, n] block; with its backward.
 * ADDITIVE to ABI 16: four new symbols, nothing existing changes, MMREC_ABI_VERSION stays 16.
 * replaces: p_g = sigmoid(n_u @ normalize(item_emb[i_id]).T), p_m = sigmoid(n_u @ normalize(it_emb[i_id]).T),
 *           mean(_kl(p_g, p_m) + _kl(p_m, p_g)) -- damrs.py, two GEMMs and about thirty elementwise launches over [m, n] blocks --
 *           and autograd's mirror of it.
 * U [m, 64], A [n, 64], B [n, 64] fp32 row-major.  With a = <U[r], A[i]>, b = <U[r], B[i]>, p = sigmoid(a), q = sigmoid(b) (the
 * sigmoid of mmrec_hardest_neg_fwd_f32: e = expf(-|z|), (z >= 0 ? 1 : e) / (1 + e)) the two divergences collapse:
 *   KL(p || q) + KL(q || p) = (p - q)(logit p - logit q) = (p - q)(a - b) =: J(a, b)
 *   out[0] = scale * sum_{r < m, i < n} J(a_ri, b_ri)                         (the caller's scale: 1 / (m n) for the mean)
 *   ga_ri  = g scale [p (1 - p)(a - b) + (p - q)],   gb_ri = -g scale [q (1 - q)(a - b) + (p - q)]      g [1] ON THE DEVICE
 *   dU = Ga A + Gb B,   dA = Ga^T U,   dB = Gb^T U                            any of dU, dA, dB may be NULL (not computed)
 * J is finite for every finite a and b; the composition it replaces is NaN (0 * log 0) once a sigmoid saturates in fp32.
 * THE PLAN.  Scores are the fp32 fma chains of the fp32-input MFMA in natural k order, the same bits in all three sweeps.
 *   forward  grid (ceil(m / 128) tiles of U) x (splits of the items); a split walks mmrec_mutual_kl_split_cols(m, n, 0) rows of
 *            A and B, staged together.  A lane adds the J of its pairs in the order it meets them (16 per 32-row sub-tile), the 64
 *            lanes of a wave by a butterfly (xor 32, 16, 8, 4, 2, 1), the four waves in order: one partial per workgroup.  The
 *            finish is ONE workgroup of 256 threads: thread t adds the partials t, t + 256, ... in order, then the same butterfly
 *            and the four waves in order, then the product with scale.
 *   backward recomputes a, b, p, q.  The dU sweep owns 128 rows of U and walks mmrec_mutual_kl_split_cols(m, n, 1) rows of A and B
 *            per split (per 32-row sub-tile: Ga A, then Gb B, into one accumulator); ONE sweep owns 128 item rows of A and B
 *            together and walks mmrec_mutual_kl_split_cols(m, n, 2) rows of U per split for dA and dB.  Products on the MFMA in
 *            the walked side's order; per-split partial gradients are added in split order.  A sweep none of whose gradients
 *            is wanted is not launched.
 * Rows past the end of a tile are zero rows: J(0, 0) = 0 and both coefficients are exactly 0, no mask anywhere.  NO ATOMICS, every
 * order fixed by (m, n) alone: two calls on the same inputs give the same bits, forward and gradients.
 * m == 0 or n == 0: out = 0 and zero gradients.  Outputs must not alias inputs.
 * workspace: mmrec_mutual_kl_workspace_bytes(m, n, d) bytes (16-byte aligned) serve either call: one float per forward workgroup;
 * for the backward the per-split partial gradients, at most 4 (m + n) 64 floats for each of dU, dA, dB.  0 for d != 64 or no pair.
 * d != 64 or a negative size: MMREC_ERR_BAD_ARG; m or n > 2^30: MMREC_ERR_UNSUPPORTED; a NULL out, a NULL U / A / B / g /
 * workspace where it is needed, dU, dA and dB all NULL: MMREC_ERR_BAD_ARG -- before any launch.  No synchronisation, no
 * allocation, no data-dependent launch shape, capture-safe, no global state. */
int32_t mmrec_mutual_kl_split_cols(int32_t m, int32_t n, int32_t mode);
size_t mmrec_mutual_kl_workspace_bytes(int32_t m, int32_t n, int32_t d);
int mmrec_mutual_kl_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d, float scale, float* out,
                        void* workspace, mmrec_stream_t stream);
int mmrec_mutual_kl_bwd_f32(const float* U, const float* A, const float* B, int32_t m, int32_t n, int32_t d, float scale,
                            const float* g, float* dU, float* dA, float* dB, void* workspace, mmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * P5 / P6  fused scoring + mask + top-K:  for every query row q: top-k over c of <Q[q], C[c]>,
 *          skipping candidates listed for q in a CSR mask (train positives), never materialising
 *          the [nq, nc] score matrix.
 * replaces: torch.matmul(u, i^T) freedom.py:219 (& bm3.py:153 layergcn.py:185 lightgcn.py:160
 *           vbpr.py:105) + scores[mask]=-1e10 + torch.topk(scores, 50) common/trainer.py:307-309 ;
 *           with Q=C=row-normalised features and k=knn_k it is the kNN build freedom.py:79-82.
 * Q [nq, kd], C [nc, kd] fp32 row-major, kd a multiple of 4.  mask_rowptr[nq+1] (int32) /
 * mask_col[...] (int32, ASCENDING within a row: the kernels binary-search it); NULL = no mask.  k <= MMREC_TOPK_MAX.
 * Output sorted by score descending (ties: lower candidate id first): out_idx[nq,k] int64,
 * out_val[nq,k] fp32 (may be NULL).  Masked candidates score -1e10 like the reference, so they can
 * only appear when fewer than k candidates are unmasked.  workspace: mmrec_topk_workspace_bytes.
 * Scores are fp32 dot products in every implementation behind this entry point: kd == 64 or 128 with >= 4096 candidates
 * runs an fp16 matrix-core FILTER with a proven error bound and rescores the ~k survivors per query exactly
 * (topk_filter.hip; `flags & MMREC_TOPK_NO_FILTER` keeps the materialised fp32 path for A/B measurements -- an
 * ARGUMENT since ABI 5: the library reads no environment and keeps no state), the other shapes materialise
 * fp32-MFMA score blocks inside the workspace (topk.hip).  Unknown flag bits: MMREC_ERR_BAD_ARG.
 * ---------------------------------------------------------------------------------------------- */
#define MMREC_TOPK_MAX 128      /* kd % 32 == 0 AND nc <= 2,097,152 candidates (full-sort evaluations, e.g. topk: [10, 20, 50, 100]; the fp16 paths serve kd = 64 / 128 up to 128 and wider rows up to 32, the fp32 block path the rest) */
#define MMREC_TOPK_MAX_OTHER 64 /* every other shape -- row widths that are not a multiple of 32, or more than 2,097,152 candidates -- runs the fused fp32 path, which ranks k <= 64: MMREC_ERR_UNSUPPORTED above it (callers fall back to their dense path; `strict_fused_eval` then raises) */
#define MMREC_TOPK_NO_FILTER 1
size_t mmrec_topk_workspace_bytes(int32_t nq, int32_t nc, int32_t kd, int32_t k);
int mmrec_score_topk_f32(const float* Q, const float* C, int32_t nq, int32_t nc, int32_t kd,
                         const int32_t* mask_rowptr, const int32_t* mask_col, int32_t k,
                         int64_t* out_idx, float* out_val, void* workspace, int32_t flags,
                         mmrec_stream_t stream);
/* Several query blocks against the SAME candidate table (ABI 7) -- the batches of one evaluation and its valid / test pair
 * (trainer.py:262,271,298-310: the item table is frozen while evaluating): the candidate side of the fp16 filter (column
 * means, centred fp16 copy of C, its norms, from 131,072 candidates on the clipping of the <= 32 rows of outlying norm:
 * 0.6 ms at 500K candidates, 8 % of a 65,536-query block) is computed once into
 * a caller-owned buffer of mmrec_topk_prepared_bytes(nc, kd) bytes (0: the filter does not serve this (nc, kd); use
 * mmrec_score_topk_f32) and handed to every call.  The buffer is valid as long as C is unchanged; same results as
 * mmrec_score_topk_f32 bit for bit.  `C` itself is still needed: the exact refinement reads the fp32 rows. */
size_t mmrec_topk_prepared_bytes(int32_t nc, int32_t kd);
int mmrec_topk_prepare_f32(const float* C, int32_t nc, int32_t kd, void* prepared, mmrec_stream_t stream);
int mmrec_score_topk_prepared_f32(const float* Q, const float* C, const void* prepared, int32_t nq, int32_t nc,
                                  int32_t kd, const int32_t* mask_rowptr, const int32_t* mask_col, int32_t k,
                                  int64_t* out_idx, float* out_val, void* workspace, int32_t flags,
                                  mmrec_stream_t stream);
/* WARM evaluation (ABI 12): the same ranking with the filter's threshold taken from a per-query LIST instead of a first pass
 * over all products -- ONE matrix-core pass per call instead of two.
 * replaces: the second and later runs of common/trainer.py:298-310 over the same users: the TEST pass that follows the VALID
 *           pass on the same frozen tables with the same train-positive mask (trainer.py:262,271; utils/dataloader.py:347,
 *           370-391), and every later epoch's evaluation, whose rankings move little from the previous one's.
 * hint [.., hint_k] int32, IN / OUT, k <= hint_k <= MMREC_TOPK_MAX (64 is the natural width for k <= 64, 128 above); hint_rows
 * (int64 [nq], may be NULL): query q uses hint row hint_rows[q] (NULL: row q) -- e.g. a table with one row per user.
 *   IN : candidate ids expected to rank high.  Any k DISTINCT, UNMASKED, in-range ids of the row bound the k-th best score from
 *        below; their approximate scores under the CURRENT Q and C give the threshold (topk_filter.hip:
 *        filter_hint_bound_kernel; with more than k usable ids the k-th largest), so the output is the exact top-k for ANY
 *        list -- bit-identical to mmrec_score_topk_f32's: a stale list only lets more candidates through to the exact
 *        refinement, a row with fewer than k usable ids (-1 padding, duplicates, masked ids) sends its query to the exact slow
 *        queue.  flags & MMREC_TOPK_HINT_COLD: the row is not read (the call runs the two-pass form) -- the FIRST evaluation.
 *   OUT: the call's own ranking of the query -- its top-k followed by the runners-up the refinement ranked anyway (up to
 *        hint_k ids, -1 beyond) -- ready to be the next call's list; flags & MMREC_TOPK_HINT_KEEP leaves the row untouched.
 * queue_counts (int32 [2] on the device, may be NULL): the call ADDS the number of queries the slow queue / the overflow queue
 * served, so that a caller can return to the cold call when its lists have gone stale.
 * prepared: as for mmrec_score_topk_prepared_f32, or NULL (the call prepares C itself).  Served shapes: those of the fp16
 * filter (kd = 64 / 128, 4096 <= nc <= 1,000,000, k <= 128); others: MMREC_ERR_UNSUPPORTED.  Other flag bits: MMREC_ERR_BAD_ARG.
 * workspace: mmrec_topk_workspace_bytes. */
#define MMREC_TOPK_HINT_COLD 1
#define MMREC_TOPK_HINT_KEEP 2
int mmrec_score_topk_hinted_f32(const float* Q, const float* C, const void* prepared, int32_t nq, int32_t nc,
                                int32_t kd, const int32_t* mask_rowptr, const int32_t* mask_col, int32_t k,
                                int32_t* hint, int32_t hint_k, const int64_t* hint_rows,
                                int64_t* out_idx, float* out_val, void* workspace, int32_t* queue_counts,
                                int32_t flags, mmrec_stream_t stream);

/* Deterministic scatter-add of per-sample gradient rows (ABI 7; config `hip_deterministic`): out[ids[b]] += rows[b], the
 * occurrences of an id summed in position order by one owner -- no float atomics, so a batch with duplicated ids gives the
 * same bits run after run (the reference's CPU scatter is deterministic).  `order` = STABLE argsort of ids
 * (int64[n], the caller sorts); ids < 0 are skipped; d a multiple of 64.  The fused backward kernels (bpr / cosine / infonce /
 * gather_scale_add) scatter with hardware fp32 atomics: in deterministic mode they are called on the batch's GATHERED rows
 * with identity ids (every output row is written once) and this entry point does the scatter into the tables. */
int mmrec_scatter_add_rows_sorted_f32(const int64_t* order, const int64_t* ids, const float* rows, int32_t n, int32_t d,
                                      float* out, mmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * P1  graph build on device.
 * replaces: get_norm_adj_mat freedom.py:102-126 (structure from de-duplicated train pairs) ;
 *           _normalize_adj_m freedom.py:145-154 ; the masked COO of pre_epoch_processing :136-143.
 * ---------------------------------------------------------------------------------------------- */
/* counts[i] += number of ids equal to i (int32 histogram, integer atomics: exact). */
int mmrec_degree_count_i32(const int64_t* ids, int64_t n, int32_t* counts, int32_t n_bins,
                           mmrec_stream_t stream);
/* per-edge symmetric normalisation: val[e] = (du[u_e]+1e-7)^-1/2 * (di[i_e]+1e-7)^-1/2 in fp32
 * (freedom.py:148-154). deg_* are int32 counts. */
int mmrec_edge_norm_f32(const int64_t* eu, const int64_t* ei, int64_t n_edges, const int32_t* deg_u,
                        const int32_t* deg_i, float* val, mmrec_stream_t stream);
/* Symmetric bipartite COO in the reference's layout cat(edges, flipped edges), cat(w, w)
 * (freedom.py:139-143): rows/cols/vals have 2*n_edges entries; item node ids are offset by n_users. */
int mmrec_bipartite_expand(const int64_t* eu, const int64_t* ei, const float* w, int64_t n_edges,
                           int32_t n_users, int32_t* rows, int32_t* cols, float* vals,
                           mmrec_stream_t stream);
/* Stable COO -> CSR: entries of a row keep their COO order (radix sort on the row key), so the SpMM
 * summation order is a pure function of the edge list.  rowptr[n_rows+1], colidx[nnz], vals_out[nnz].
 * workspace: mmrec_coo_to_csr_workspace_bytes(nnz, n_rows). */
size_t mmrec_coo_to_csr_workspace_bytes(int64_t nnz, int32_t n_rows);
int mmrec_coo_to_csr(const int32_t* rows, const int32_t* cols, const float* vals, int64_t nnz,
                     int32_t n_rows, int32_t* rowptr, int32_t* colidx, float* vals_out,
                     void* workspace, mmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Rows next to the hot path.
 * ---------------------------------------------------------------------------------------------- */
/* f1  one uniform negative per sample from cand_items[n_cand] (train-seen items), rejected while it
 * is in the user's training history (CSR hist_rowptr/hist_col, item ids sorted inside a row).
 * replaces: TrainDataLoader._sample_neg_ids utils/dataloader.py:267-275 (python `random` loop).
 * Counter-based RNG: reproducible, but not the host stream -- the host sampler remains the bit-exact
 * parity mode.  With mix64 = splitmix64's output function and G = 0x9E3779B97F4A7C15, sample b starts
 * from the state s = mix64(mix64(mix64(seed + G) + counter) + b); draw t = 1, 2, ... is mix64(s + t G), its
 * high 32 bits r select cand_items[(r * n_cand) >> 32].  At most 4096 draws per sample: a user whose
 * history holds every candidate gets the item of the 4096th draw.  (The three mixing rounds replace
 * s = seed ^ (counter C + b G), under which a small seed -- 0 is the loader's default -- made sample
 * b + 1's draws repeat sample b's, one draw late.  The ids for a given (seed, counter) therefore
 * differ from earlier builds of ABI 16; the stream was never part of the ABI.) */
int mmrec_sample_negatives_i64(const int64_t* users, int32_t batch, const int32_t* hist_rowptr,
                               const int32_t* hist_col, const int32_t* cand_items, int32_t n_cand,
                               uint64_t seed, uint64_t counter, int64_t* out_neg,
                               mmrec_stream_t stream);
/* f2  hit matrix + per-user Recall / NDCG / Precision / MAP at the cut-offs ks[n_ks] (ascending,
 * <= k) from the top-k ids and the ground-truth CSR (item ids sorted inside a row).
 * replaces: the Python double loop topk_evaluator.py:88-93 and the per-user part of metrics.py:12-105.
 * discount[j] = 1/log2(j+2), idcg_cum[j] = cumulative sum of discount (host-computed doubles, k
 * entries).  Per-user sums run sequentially in the order of numpy's cumsum: out_per_user[u][m][t]
 * (m: 0 recall, 1 ndcg, 2 precision, 3 map) is bit-identical to the reference's per-user value.
 * A user without ground truth (an empty row) gets what the reference's formulas give there: recall
 * NaN (0 / 0), and ndcg = 0 / idcg_cum[k-1], precision = 0 / (j + 1) and map = 0 / k, all 0.0.
 * hit_out [n_users, k] uint8 may be NULL. */
int mmrec_topk_metrics_f64(const int64_t* topk_idx, int32_t n_users, int32_t k,
                           const int32_t* gt_rowptr, const int32_t* gt_col, const double* discount,
                           const double* idcg_cum, const int32_t* ks, int32_t n_ks, uint8_t* hit_out,
                           double* out_per_user, mmrec_stream_t stream);

/* f3  fused dense Adam step on one tensor (16-byte aligned): exp_avg / exp_avg_sq updated in place,
 * bias corrections from `step` (>= 1), optional L2 weight_decay folded into the gradient.
 * replaces: torch.optim.Adam.step common/trainer.py:111-128,189 (same update formula). */
int mmrec_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int64_t step,
                        mmrec_stream_t stream);

/* Graph-replay-safe Adam: the step count (int64) and the learning rate (fp32) live in device memory.
 * mmrec_adam_prepare increments *step_dev and writes hyper_dev[2] = {lr/(1-b1^t), 1/sqrt(1-b2^t)} once
 * per optimizer step; mmrec_adam_step_dev_f32 applies the update to one tensor reading hyper_dev.  A
 * captured hipGraph of a training step therefore replays with correct bias corrections. */
int mmrec_adam_prepare(int64_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_dev,
                       mmrec_stream_t stream);
int mmrec_adam_step_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                            float beta1, float beta2, float eps, float weight_decay,
                            mmrec_stream_t stream);

/* Multi-tensor Adam: ALL parameter tensors of one optimizer step in one launch per 24 tensors (a training
 * step otherwise pays 8-32 tiny launches).  p / g / m / v / n (and lr / step) are HOST arrays of n_tensors
 * entries holding device pointers and element counts; the table is copied into the kernel-argument segment,
 * so the arrays only need to live for the call.  Entries with n == 0 are skipped.  Same update as
 * mmrec_adam_step_f32 (per-tensor lr and step, as torch keeps them) / mmrec_adam_step_dev_f32 (one device
 * hyper pair for all tensors: call mmrec_adam_prepare first).
 * replaces: torch.optim.Adam.step common/trainer.py:111-128,189. */
int mmrec_adam_multi_step_f32(float* const* p, const float* const* g, float* const* m, float* const* v,
                              const int64_t* n, int32_t n_tensors, const float* lr, const int64_t* step,
                              float beta1, float beta2, float eps, float weight_decay, mmrec_stream_t stream);
int mmrec_adam_multi_step_dev_f32(float* const* p, const float* const* g, float* const* m, float* const* v,
                                  const int64_t* n, int32_t n_tensors, const float* hyper_dev, float beta1,
                                  float beta2, float eps, float weight_decay, mmrec_stream_t stream);

/* a14  HOST function (no GPU involved): the reference's negative sampler bit for bit.  Continues CPython's Mersenne
 * Twister from `random.getstate()` (mt_state[624] + *mt_index, both updated in place) and draws, per user of the batch,
 * `all_items[_randbelow(n_all_items)]` until the item is not in the user's history (hist_rowptr [n_users + 1] /
 * hist_items ascending per user, int64) -- the exact output sequence and stream consumption of
 * `_sample_neg_ids` dataloader.py:267-275 (`random.sample(self.all_items, 1)[0]` in a rejection loop).
 * replaces: the per-sample Python loop (0.75 ms per 2048-user batch; ~10 us here). */
int mmrec_host_sample_negatives(uint32_t* mt_state, int32_t* mt_index, const int64_t* users, int32_t batch,
                                const int64_t* hist_rowptr, const int64_t* hist_items, const int64_t* all_items,
                                int32_t n_all_items, int64_t* out);

/* a4  HOST function: `random.sample(range(n), k)` of CPython 3.10 bit for bit (same result list, same generator state
 * afterwards) -- the uniform edge pruning of LayerGCN's alternate epochs, layergcn.py:56-58.  mt_state / mt_index as in
 * mmrec_host_sample_negatives; out [k] int64; scratch [n] int32. */
int mmrec_host_random_sample_range(uint32_t* mt_state, int32_t* mt_index, int32_t n, int32_t k, int64_t* out,
                                   int32_t* scratch);

/* a9'  BM3's BYOL terms: out[0] = scale * sum_b cos(X[ix[b]], Y[iy[b]]) with F.cosine_similarity's clamp (each norm at
 * least 1e-8); rows of d = 64 j floats; ix / iy NULL = row b.  The targets are detached in the reference, so the backward
 * produces the gradient w.r.t. X only: dX[ix[b]] += grad * scale * dcos_b/dx (atomic: duplicate ids).  coef [batch][2] fp32
 * and workspace (mmrec_cosine_workspace_bytes) are written by the forward, coef is read by the backward.
 * replaces: the six `1 - cosine_similarity(p, z.detach(), dim=-1).mean()` terms bm3.py:129-144 (and selfcfed_lgn.py:57-58). */
size_t mmrec_cosine_workspace_bytes(int32_t batch);
int mmrec_cosine_fwd_f32(const float* X, const int64_t* ix, const float* Y, const int64_t* iy, int32_t batch, int32_t d,
                         float scale, float* out, float* coef, void* workspace, mmrec_stream_t stream);
int mmrec_cosine_bwd_f32(const float* X, const int64_t* ix, const float* Y, const int64_t* iy, int32_t batch, int32_t d,
                         const float* coef, const float* grad_scalar, float scale, float* dX, mmrec_stream_t stream);

/* f3  Row-lazy EXACT Adam for a trainable [n_rows, F] table of which a step touches few rows (F % 4 == 0).  Rows
 * with a zero gradient are not visited; their postponed updates (dense-Adam semantics: the moments keep decaying,
 * the parameter keeps moving) are replayed in registers, with the dense kernel's instructions in its order, when the
 * row is next needed -- results equal the dense update bit for bit.
 *   hist     [capacity][2] fp32: step-dependent scalars of optimizer step t, written by mmrec_adam_hist_set(t)
 *   last_step[n_rows] int32: steps already applied per row (0 initially)
 *   ids may hold -1 = "no row" (a slot served elsewhere, e.g. by another rank's shard of the table): skipped everywhere.
 *   owner    [n_rows] int32, INT_MAX where idle: mmrec_adam_rows_owner marks the first position of every row in `ids`
 *            (duplicates allowed); catchup / step consume the marks (entries are INT_MAX again afterwards)
 *   catchup: bring the rows of `ids` (ids == NULL: all n_rows rows) to step t_now
 *   step:    optimizer step t (= t_now + 1) on the rows of `ids`; g [n_ids][F]: row i holds the gradient of OCCURRENCE i;
 *            the occurrences of a table row are summed in position order by the workgroup of its first occurrence
 *            (n_ids <= MMREC_ADAM_ROWS_MAX_IDS: the position list lives in LDS).  presummed != 0: row i already holds the
 *            SUMMED gradient of the table row whose first occurrence is position i (other positions are ignored)
 * replaces: torch.optim.Adam.step on image_embedding / text_embedding (freedom.py:58,61; trainer.py:111-128,189). */
#define MMREC_ADAM_ROWS_MAX_IDS 16000
int mmrec_adam_hist_set(float* hist, int32_t t, float lr, float beta1, float beta2, mmrec_stream_t stream);
int mmrec_adam_rows_owner(const int64_t* ids, int32_t n, int32_t* owner, mmrec_stream_t stream);
int mmrec_adam_rows_catchup_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, int32_t n_ids,
                                int32_t n_rows, int32_t F, int32_t* last_step, const float* hist, int32_t t_now,
                                float beta1, float beta2, float eps, float weight_decay, mmrec_stream_t stream);
int mmrec_adam_rows_step_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, const float* g,
                             int32_t n_ids, int32_t F, int32_t* last_step, int32_t t, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int32_t presummed, mmrec_stream_t stream);
/* The same three calls for a step replayed as a hipGraph (hip_graph_step): nothing step-dependent comes from the host.
 * step_dev [1] int64 and hyper_dev [2] fp32 are the device scalars mmrec_adam_prepare maintains (step count; lr / (1 -
 * b1^t), 1 / sqrt(1 - b2^t)).  Order inside a step: catchup_dev (before prepare: step_dev = steps taken so far) ...
 * backward ... mmrec_adam_prepare ... hist_set_dev ... rows_step_dev.  hist_set_dev does not write beyond `capacity`
 * entries: it raises *overflow (sticky, device int32) instead, which the host checks between epochs; from then on
 * catchup_dev / rows_step_dev (ABI 7: they take the same `capacity`) leave the rows untouched -- there is no table entry to
 * replay from -- so the run can be resumed from the state before the overflowing step.  Such a refused call returns before
 * it looks at a row, so the marks mmrec_adam_rows_owner made for it are NOT released: whoever resumes refills `owner` with
 * INT_MAX first (LazyRowEmbedding.resume does).  hist[capacity - 1] is the last entry ever written. */
int mmrec_adam_hist_set_dev(float* hist, int32_t capacity, const int64_t* step_dev, const float* hyper_dev,
                            int32_t* overflow, mmrec_stream_t stream);
int mmrec_adam_rows_catchup_dev_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, int32_t n_ids,
                                    int32_t n_rows, int32_t F, int32_t* last_step, const float* hist, int32_t capacity,
                                    const int64_t* step_dev, float beta1, float beta2, float eps, float weight_decay,
                                    mmrec_stream_t stream);
int mmrec_adam_rows_step_dev_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, const float* g,
                                 int32_t n_ids, int32_t F, int32_t* last_step, int32_t capacity, const int64_t* step_dev,
                                 const float* hyper_dev, float beta1, float beta2, float eps, float weight_decay,
                                 int32_t presummed, mmrec_stream_t stream);
/* ABI 13 -- OPT-IN fast-forward (config key `lazy_adam_fast_forward`, default off): the arguments and the bookkeeping of
 * catchup / catchup_dev, but a row skipped for more than 12 steps is brought to step t_now in CLOSED FORM instead of being
 * replayed step by step: m *= b1^n, v *= b2^n, p -= m0 * sum_j w_j / (sqrt(v0) d_j + eps) with the sum evaluated as a
 * six-term series around the row's weighted-mean d (csrc/adam.hip; the row scalars W, dbar, M_2..M_6 come from `hist`).
 * ~16 instructions per element whatever the gap (the exact replay: 7 per element AND skipped step).  NOT bit-identical to
 * dense Adam: p within 2e-6 of the distance it moved, m / v within 1e-6 sqrt(n) relative (tests) -- inside north_star's
 * 1e-4 tolerance, outside the "lazy == dense bit for bit" property, hence opt-in.  What the series does not serve to 1e-7
 * (steps before optimizer step 128, where the bias correction of v moves by per cents per step: such a row is replayed to
 * step 128 and advanced in closed form from there; b1^256 > 1e-9; weight decay; short gaps) takes the exact replay inside
 * the same launch.
 * replaces: the same torch.optim.Adam.step as above (trainer.py:111-128,189). */
int mmrec_adam_rows_fastforward_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, int32_t n_ids,
                                    int32_t n_rows, int32_t F, int32_t* last_step, const float* hist, int32_t t_now,
                                    float beta1, float beta2, float eps, float weight_decay, mmrec_stream_t stream);
int mmrec_adam_rows_fastforward_dev_f32(float* p, float* m, float* v, const int64_t* ids, int32_t* owner, int32_t n_ids,
                                        int32_t n_rows, int32_t F, int32_t* last_step, const float* hist,
                                        int32_t capacity, const int64_t* step_dev, float beta1, float beta2, float eps,
                                        float weight_decay, mmrec_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMREC_HIP_H */
