/*
 * lpformer_hip.h -- C ABI of the MI355X (gfx950) LPFormer link-scoring library.
 *
 * Two shared objects export these symbols:
 *   liblpformer_hip.so   (hipcc, --offload-arch=gfx950)  every entry point taking a stream
 *   liblpformer_host.so  (g++ -fopenmp)                   lpf_ppr_push_cpu, lpf_ppr_push_cpu_sources, lpf_host_free, lpf_host_abi_version
 *
 * The reference (HarryShomer/LPFormer) is 100 % Python and has no FFI of its own; each entry point
 * below therefore cites the reference Python it replaces (paths relative to the reference repo root)
 * and INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer (device pointers unless a name ends in
 *     _host); no allocation, no exceptions, no hidden state: re-entrant per stream.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  Nothing synchronises the host
 *     (graph-capturable) -- except the *_host functions, which run on the calling thread(s).
 *   - return value: LPF_OK or a negative LPF_ERR_* code; lpf_strerror() names it.
 *   - CSR graphs: rowptr int64[n+1], col int32[nnz] sorted ascending inside each row, no duplicates.
 *   - feature matrices are row-major fp32 with an explicit leading dimension (in elements).
 *   - fp32 rows handed to the GEMM must be 16-byte aligned with ld % 4 == 0.
 */
#ifndef LPFORMER_HIP_H
#define LPFORMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPF_OK 0
#define LPF_ERR_INVALID (-1)     /* bad argument (null pointer, size, alignment)        */
#define LPF_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for        */
#define LPF_ERR_LAUNCH (-3)      /* hipLaunch / runtime error (see lpf_last_hip_error)  */
#define LPF_ERR_NO_DEVICE (-4)   /* no gfx950 device visible                            */

#define LPF_ABI_VERSION 16

/* GEMM / row-wise epilogue flags */
#define LPF_FLAG_RELU 1u

int lpf_abi_version(void);
const char *lpf_strerror(int code);
/* Last HIP runtime error string seen by this library on the calling thread ("" if none). */
const char *lpf_last_hip_error(void);
/* Fills cu_count / lds_bytes_per_cu / wave_size of the current device; LPF_ERR_NO_DEVICE if none. */
int lpf_device_info(int *cu_count, int *lds_bytes_per_cu, int *wave_size, char *arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------------
 * Encoder (reference: src/models/other_models.py:61-76 GCN.forward -> torch_geometric GCNConv;
 *          src/models/link_transformer.py:110-129 propagate)
 * ---------------------------------------------------------------------------------------------- */

/* GCN symmetric normalisation on a CSR that already CONTAINS every diagonal entry
 * (replaces torch_geometric.nn.conv.gcn_conv.gcn_norm, called from other_models.py:35,66):
 *   w'_ij = (i==j ? 1 : w_ij);  deg_i = sum_j w'_ij;  w_out_ij = deg_i^-1/2 * w'_ij * deg_j^-1/2 (inf -> 0).
 * w_in may be NULL (all ones).  dis_tmp: n floats of scratch (receives deg^-1/2). */
int lpf_gcn_norm_csr(int64_t n, const int64_t *rowptr, const int32_t *col, const float *w_in,
                     float *w_out, float *dis_tmp, void *stream);

/* out[i,:] = epilogue( sum_j w_ij * H[col_ij,:] )   -- GCNConv.propagate + everything up to the next layer
 * (other_models.py:66-74 and, for the last layer, link_transformer.py:127):
 *   y = acc + bias;  if ln_g: y = LN(y; ln_g, ln_b);  if RELU: y = max(y,0);
 *   if residual: y = residual[i,:] + y;  if ln2_g: y = LN(y; ln2_g, ln2_b)
 * D % 4 == 0, D <= 256.  bias, ln_g, ln_b, residual, ln2_g, ln2_b may each be NULL.
 * long_rows (optional, NULL/0 = none): int32[n_long] list of EVERY row with more than LPF_SPMM_LONG_ROW stored entries
 * (row ids relative to `rowptr`); those hub rows get a whole workgroup each instead of one lane group. */
#define LPF_SPMM_LONG_ROW 128
int lpf_spmm_csr_f32(int64_t n, int32_t D, const int64_t *rowptr, const int32_t *col, const float *w,
                     const float *H, int64_t ldh, float *out, int64_t ldo, const float *bias,
                     const float *ln_g, const float *ln_b, const float *residual, int64_t ldr,
                     const float *ln2_g, const float *ln2_b, uint32_t flags, const int32_t *long_rows,
                     int64_t n_long, void *stream);

/* One GCN layer in one launch, square case (in = out = D in {32, 64, 128}): aggregate first, transform in registers
 * (gcn_fused.hip).  Replaces lpf_gemm_f32 + lpf_spmm_csr_f32 for such a layer (other_models.py:61-76 -> GCNConv):
 *   out[r - row_base] = epilogue( (sum_e w_e H[col_e]) W^T ),  epilogue = + bias, LayerNorm, ReLU, + residual, gnn_norm
 * as lpf_spmm_csr_f32 (same flags).  row_order int32[16 n_tiles]: the rows to produce, in the order they are worked on
 * -- any order is correct; lpformer_amd/graph.py fused_row_order sorts by degree so that the 16 rows of a tile, which
 * advance in lockstep, are equally long -- with -1 = padding and v <= -2 = hub number (-2 - v): hubs int32[n_hub][3] =
 * (row id, first slice, number of slices), the hub row's entry list being replaced by rows first .. first + number - 1
 * of t_parts (float[n_slices][D], lpf_spmm_row_parts_f32), each with weight 1.  rowptr is indexed by the global row
 * id; out / residual hold rows row_base...  w_packed = the weight image of lpformer_amd/fold.py pack_dense(W, 1)
 * (W = GCNConv.lin.weight, [D, D]).  pre_out (optional, training): receives the rows before the LayerNorm (product +
 * bias), what a LayerNorm backward needs.  Rounding order differs from transform-then-aggregate (A (X W^T) vs
 * (A X) W^T); identical from launch to launch. */
int lpf_gcn_layer_fused_f32(int32_t D, int64_t n_tiles, const int32_t *row_order, int64_t row_base,
                            const int64_t *rowptr, const int32_t *col, const float *w, const float *H, int64_t ldh,
                            const float *w_packed, float *out, int64_t ldo, const float *bias, const float *ln_g,
                            const float *ln_b, const float *residual, int64_t ldr, const float *ln2_g,
                            const float *ln2_b, uint32_t flags, const int32_t *hubs, const float *t_parts,
                            float *pre_out, int64_t ldpre, void *stream);
/* The layer as the TRAINING forward and backward launch it (lpformer_amd/train.py GcnFusedFn; reference: the autograd
 * graph of GCNConv + LayerNorm + ReLU + dropout + residual, src/models/other_models.py:61-76): no second LayerNorm, and
 *   agg_out (optional, float[n][ldagg]) receives the AGGREGATED rows sum_e w_e H[col_e] the product is taken of -- what
 *     the weight gradient dW = dU^T agg needs;
 *   drop_p > 0: F.dropout behind the ReLU (other_models.py:69), in the kernel -- element (row, feature) is kept and scaled
 *     by 1 / (1 - drop_p) iff a counter-based hash of (drop_seed, row, feature) passes p (csrc/lpf_common.h
 *     lpf_drop_bits: no mask tensor; lpf_layernorm_relu_drop_bwd_f32 recomputes it); then residual (optional) is added.
 * out = residual + dropout(ReLU(LN((A H) W^T + bias))).  The backward launches it once more over the transposed graph
 * with the transposed weight image, no epilogue, residual = the gradient that arrived through the skip connection:
 * dX = dOut + (A^T dU) W. */
int lpf_gcn_layer_fused_train_f32(int32_t D, int64_t n_tiles, const int32_t *row_order, int64_t row_base,
                                  const int64_t *rowptr, const int32_t *col, const float *w, const float *H, int64_t ldh,
                                  const float *w_packed, float *out, int64_t ldo, const float *bias, const float *ln_g,
                                  const float *ln_b, const float *residual, int64_t ldr, uint32_t flags,
                                  const int32_t *hubs, const float *t_parts, float *pre_out, int64_t ldpre,
                                  float *agg_out, int64_t ldagg, float drop_p, uint64_t drop_seed, void *stream);
/* The same layer gathering from a bf16 table (the bf16-table encoder mode; D = 64 or 128).  H_bf16p: uint16 rows, ldh in
 * elements (a multiple of 8), in the PERMUTED order  element 32 i + 8 q + 4 h + u = feature 16 (2 i + h) + 4 q + u
 * (i < D/32, q < 4, h < 2, u < 4) -- a lane's 16-byte load then holds two whole 16-feature k-groups.  out receives the
 * fp32 rows in normal order; out_bf16p (optional, ldob in elements) the same rows as permuted bf16, i.e. the next
 * layer's table.  Hub rows must sit in tiles of their own (fused_row_order(..., pad_hubs=True)); their slices come
 * from lpf_spmm_row_parts_bf16p, which reads the permuted table and writes fp32 sums in normal order. */
int lpf_gcn_layer_fused_bf16(int32_t D, int64_t n_tiles, const int32_t *row_order, int64_t row_base,
                             const int64_t *rowptr, const int32_t *col, const float *w, const void *H_bf16p,
                             int64_t ldh, const float *w_packed, float *out, int64_t ldo, const float *bias,
                             const float *ln_g, const float *ln_b, const float *residual, int64_t ldr,
                             const float *ln2_g, const float *ln2_b, uint32_t flags, const int32_t *hubs,
                             const float *t_parts, void *out_bf16p, int64_t ldob, void *stream);
int lpf_spmm_row_parts_bf16p(int32_t D, const int64_t *parts, int64_t n_parts, const int32_t *col, const float *w,
                             const void *H_bf16p, int64_t ldh, float *out, void *stream);

/* Sums of slices of (hub) rows: out[p][:D] = sum over the stored entries e in [parts[2p], parts[2p+1]) of w_e H[col_e]
 * (one workgroup per slice, partial sums added in a fixed order).  D a multiple of 8, <= 128. */
int lpf_spmm_row_parts_f32(int32_t D, const int64_t *parts, int64_t n_parts, const int32_t *col, const float *w,
                           const float *H, int64_t ldh, float *out, void *stream);

/* bf16 THROUGHPUT MODE of the aggregation (BASELINE.json config 2 names bf16 storage; SURVEY 8b lpf_spmm_csr_bf16):
 * the gathered table H holds bf16 rows (ldh in bf16 elements, rows 16-byte aligned) -- half the gather bytes, which
 * are what bounds this kernel --, the sum over neighbours, the epilogue and the output stay fp32 (D % 8 == 0: a lane
 * gathers 8 bf16 = 16 bytes, so a row needs half the lanes of the fp32 kernel).  The table comes
 * from lpf_gemm_f32_out_bf16 (the layer's X W^T, rounded to nearest even once). */
int lpf_spmm_csr_bf16(int64_t n, int32_t D, const int64_t *rowptr, const int32_t *col, const float *w,
                      const void *H_bf16, int64_t ldh, float *out, int64_t ldo, const float *bias,
                      const float *ln_g, const float *ln_b, const float *residual, int64_t ldr,
                      const float *ln2_g, const float *ln2_b, uint32_t flags, const int32_t *long_rows,
                      int64_t n_long, void *stream);

/* C[M,N] = A[M,K] * W[N,K]^T (+ bias[N]) (+ addend[M,N]) (ReLU)   -- nn.Linear / PyG Linear:
 * GCNConv.lin (other_models.py:66), lin_l / node half of lin_r (src/modules/layers.py:206-214),
 * MLP linears (other_models.py:125-138), mlp_score (other_models.py:173-179).
 * fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 accumulate.  lda, ldw % 4 == 0; bias/addend may be NULL. */
int lpf_gemm_f32(int64_t M, int32_t N, int32_t K, const float *A, int64_t lda, const float *W, int64_t ldw,
                 const float *bias, const float *addend, int64_t ldadd, float *C, int64_t ldc,
                 uint32_t flags, void *stream);
/* Same product, C stored as bf16 (ldc in bf16 elements). */
int lpf_gemm_f32_out_bf16(int64_t M, int32_t N, int32_t K, const float *A, int64_t lda, const float *W, int64_t ldw,
                          const float *bias, const float *addend, int64_t ldadd, void *C_bf16, int64_t ldc,
                          uint32_t flags, void *stream);

/* C[N,K] = A[M,N]^T * B[M,K]   -- the weight gradient of a Linear layer (dW = dY^T X; the training step,
 * src/train/train_model.py:59-77 through autograd).  The reduction over the M rows is split into chunks whose partial
 * products are added in chunk order (deterministic).  workspace: lpf_gemm_tn_workspace_floats(M, N, K) floats. */
int64_t lpf_gemm_tn_workspace_floats(int64_t M, int32_t N, int32_t K);
int lpf_gemm_tn_f32(int64_t M, int32_t N, int32_t K, const float *A, int64_t lda, const float *B, int64_t ldb,
                    float *C, int64_t ldc, float *workspace, void *stream);
/* The same product with the column sums of A beside it: colsum[n] = sum_m A[m][n] -- the bias gradient of the Linear
 * layer whose weight gradient C is (dY^T X and dY^T 1 in one pass over dY; replaces a lpf_colsum_f32 launch pair per
 * layer of the training step).  Same workspace. */
int lpf_gemm_tn_colsum_f32(int64_t M, int32_t N, int32_t K, const float *A, int64_t lda, const float *B, int64_t ldb,
                           float *C, int64_t ldc, float *colsum, float *workspace, void *stream);

/* y[i,:] = LN(x[i,:]; g, b) (then ReLU if flagged), in place allowed (nn.LayerNorm eps 1e-5, biased variance).
 * other_models.py:131-132, layers.py:78.  D <= 1024. g/b NULL -> plain ReLU / identity. */
int lpf_layernorm_f32(int64_t M, int32_t D, const float *x, int64_t ldx, const float *g, const float *b,
                      float *y, int64_t ldy, uint32_t flags, void *stream);

/* Backward of lpf_layernorm_f32 (no ReLU): dx, dgamma, dbeta from x, dy, gamma (row statistics recomputed from x;
 * column sums added in a fixed order).  D % 4 == 0, D <= 256; workspace: lpf_layernorm_bwd_workspace_floats(D) floats.
 * The training step (src/train/train_model.py:59-77 through autograd). */
int64_t lpf_layernorm_bwd_workspace_floats(int32_t D);
/* The same for y = ReLU(LN(x)) (the GCN layer's epilogue, other_models.py:66-69, and the MLPs' hidden layers, :131-133):
 * dy counts only where gamma xhat + beta > 0; dxsum[D] = column sums of dx, the gradient of a bias added in front of
 * the LayerNorm.  Same workspace. */
int lpf_layernorm_relu_bwd_f32(int64_t M, int32_t D, const float *x, int64_t ldx, const float *dy, int64_t ldy,
                               const float *gamma, const float *beta, float *dx, int64_t lddx, float *dgamma,
                               float *dbeta, float *dxsum, float *workspace, void *stream);
/* The same backward behind the in-kernel dropout of lpf_gcn_layer_fused_train_f32: the forward was
 * y = dropout(ReLU(LN(x))) with (drop_p, drop_seed); dy is scaled by 1 / (1 - drop_p) where (row, feature) was kept and
 * dropped where it was not -- the mask is recomputed from the seed (rows are numbered from 0). */
int lpf_layernorm_relu_drop_bwd_f32(int64_t M, int32_t D, const float *x, int64_t ldx, const float *dy, int64_t ldy,
                                    const float *gamma, const float *beta, float drop_p, uint64_t drop_seed, float *dx,
                                    int64_t lddx, float *dgamma, float *dbeta, float *dxsum, float *workspace,
                                    void *stream);
int lpf_layernorm_bwd_f32(int64_t M, int32_t D, const float *x, int64_t ldx, const float *dy, int64_t ldy,
                          const float *gamma, float *dx, int64_t lddx, float *dgamma, float *dbeta, float *workspace,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pair stage (reference: src/models/link_transformer.py:132-178 calc_pairwise and helpers)
 * ---------------------------------------------------------------------------------------------- */

/* mul[k,:] = X[a_k,:] * X[b_k,:]  and  sum[k,:] = X[a_k,:] + X[b_k,:]   (link_transformer.py:101-102,143).
 * With X = Y := X_node W_l^T + b_l (one GEMM per encoder output) the sum IS the attention query of the pair,
 * lin_l(xa) + lin_l(xb) (layers.py:212-215): no per-pair GEMM.
 * batch: int64 [2, bs] row-major (row 0 = a, row 1 = b) with row stride `batch_ld`.  mul or sum may be NULL.
 * n_rows: rows of X; an id outside [0, n_rows) reads row 0 instead (lpf_select_plan raises LPF_SELECT_ERR_NODE_RANGE
 * for such a batch; the reference raises an index error at link_transformer.py:101). */
int lpf_pair_gather_f32(int64_t bs, int32_t D, const int64_t *batch, int64_t batch_ld, int64_t n_rows, const float *X,
                        int64_t ldx, float *mul, int64_t ldm, float *sum, int64_t lds, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Selection, GENERAL path (select2.hip; a caller-supplied typing adjacency -- for the model's own adjacency see
 * lpf_select3_* below): two launches, nothing read back by the host.
 * compute_node_mask + get_ppr_vals + get_non_1hop_ppr (link_transformer.py:214-319,434-481), eval mode; bit-exact.
 * The candidates of the batch form one flat slot space -- pair k owns N(a_k) | N(b_k) | the shorter of the two T0
 * rows, at least one slot -- cut into work items of LPF_SELECT_ITEM slots; one thread per slot.
 *
 *   ctl   int64[LPF_SELECT_CTL_WORDS], zero-initialised once by the caller, then owned by the library; ONE batch size
 *         per control block (the launch number is derived from the plan ticket):
 *         [0] slots of the batch  [1] work items  [2] item ticket  [3] STICKY error bits (LPF_SELECT_ERR_*; the caller
 *         clears them after handling)  [4..6] selected entries per type (cn, 1-hop, >1-hop)  [7] plan ticket
 *         [8] launch number (tags the chained-scan words: those of earlier launches read as "not ready", nothing is
 *         ever cleared and no per-launch value comes from the host, so the two launches replay from a captured graph)
 *   desc  128 bytes per pair;  offs int64[bs+1];  item_pair int32[item_cap];  plan_lb uint64[lpf_select_plan_blocks(bs)]
 *   run_lb uint64[3*item_cap];  type_ptr int32[3*(bs+1)];  entries 16 bytes x 3 x ent_cap
 *   val_*  the rows PPR values are looked up in: the raw PPR matrix, plain sorted CSR (val_rowptr / val_col / val_val;
 *          val_len NULL).  adj_selfp and val_cv must be NULL: round 2's indexed form of this call (self-PPR aligned
 *          with the adjacency + a hashed one-hop index) was superseded by lpf_select3_* and returns LPF_ERR_UNSUPPORTED
 *   BLOCKED index (the T0 rows): every row padded to a multiple of 16 entries (column INT32_MAX, value 0), row
 *          pointers counting padded entries, t0_len[i] = real entries of row i, t0_cv = interleaved {int32 column,
 *          float value} pairs (a 16-entry block = one aligned 128-byte line), t0_skip[b] = last column of block b
 *          (+ 40 spare entries): a lookup reads the row's skip entries, then one block that carries the value.
 *   HASHED index (the P1 rows with adj_selfp): row i owns val_len[i] buckets of 8 {column, value} entries (val_cv,
 *          64 aligned bytes per bucket, unused entries column INT32_MAX), val_rowptr counting entries
 *          (8 per bucket); entry (i, c) sits in bucket  mulhi_u32(c * 2654435761 mod 2^32, val_len[i])  and no
 *          bucket overflows (the builder grows a row's bucket count until that holds): ONE memory round trip per
 *          lookup.  Without adj_selfp (adjacency override) val_col / val_val are the raw PPR rows, plain sorted CSR.
 *   adjx_* UNMASKED adjacency for the >1-hop exclusion (link_transformer.py:443); NULL = the typing adjacency
 * Result: per type t a dense region entries[t*ent_cap ..) of {pair | from_N(b) << 31, node, pa, pb} records ordered by
 * (pair, candidate slot); segment of pair k = [type_ptr[t*(bs+1)+k], type_ptr[t*(bs+1)+k+1]); the one-hop segment
 * lists the kept nodes of N(a), then those of N(b).  Entries past ent_cap are dropped and LPF_SELECT_ERR_ENTRY_CAP is
 * raised; consumers clamp to ent_cap.  grid_blocks: persistent workgroups of the run kernel (0 = default).
 * mode_cn (lpf_select_run): mask mode "cn" (link_transformer.py:39-44,232-247) -- common neighbours only, their round
 * trip with t = 1, thresh_cn filter; pass t0_* = NULL with it (no >1-hop nodes). */
#define LPF_SELECT_ITEM 1024
#define LPF_SELECT_CTL_WORDS 16
#define LPF_SELECT_ERR_NODE_RANGE 1 /* a node id of the batch is outside [0, n_nodes): the pair was treated as empty */
#define LPF_SELECT_ERR_ITEM_CAP 2   /* more work items than item_cap: the batch was not processed completely      */
#define LPF_SELECT_ERR_ENTRY_CAP 4  /* more selected entries of one type than ent_cap                              */
int64_t lpf_select_plan_blocks(int64_t bs);
int lpf_select_plan(int64_t bs, const int64_t *batch, int64_t batch_ld, int64_t n_nodes, const int64_t *adj_rowptr,
                    const int64_t *val_rowptr, const int64_t *t0_rowptr, const int64_t *adjx_rowptr,
                    const int32_t *val_len, const int32_t *t0_len, void *desc, int64_t *offs, int32_t *item_pair,
                    int64_t item_cap, int64_t *ctl, uint64_t *plan_lb, void *stream);
int lpf_select_run(int64_t bs, const void *desc, const int64_t *offs, const int32_t *item_pair, int64_t item_cap,
                   int64_t *ctl, uint64_t *run_lb, const int32_t *adj_col, const float *adj_selfp,
                   const int32_t *adjx_col, const int32_t *val_col, const float *val_val, const void *val_cv,
                   const void *t0_cv, const int32_t *t0_skip, float th_cn, float th_1hop,
                   float th_non1hop, int32_t mode_cn, int32_t *type_ptr, void *entries, int64_t ent_cap,
                   int32_t grid_blocks, void *stream);
/* Selection over the per-model WALK INDEXES (select3.hip) -- the evaluation path: the typing adjacency is the model's
 * own adj_mask / full_adj_mask (link_transformer.py:226-227 with adj=None), mask modes "all", "1-hop" and "cn"
 * (:39-44).  Same control block, workspaces, result layout and error bits as lpf_select_plan / lpf_select_run above
 * (which remain the path for a caller-supplied adjacency override); desc is 128 bytes per pair, a pair owns at least
 * 16 slots.  Every selected set is an intersection evaluated from its shorter side with one hashed look-up per
 * candidate.  Index arrays, built once per (adjacency, PPR matrix, thresholds) by
 * lpformer_amd/graph.py build_walk_index; "cv" = interleaved {int32 node, fp32 value bits} pairs:
 *   node_rec 64 bytes per node: int64 {adj0, a10, px0, t00, u0} element offsets of the node's rows in adj_cv, a1_cv,
 *            px_cv, t0_cv (entries) and u_cv (entries, 8 per bucket), int32 {deg, n_a1, n_px, n_t0, u_buckets, 0}
 *   adj_cv   the adjacency rows with selfp[e] = P[i, j] (0 where the PPR matrix stores nothing)
 *   a1_cv    the adjacency entries whose own value passes the one-hop test fl32(fl32(p+1)-1) >= theta_1
 *   px_cv    the PPR entries (i, v), v NOT adjacent to i, that pass the weaker of the one-hop / >1-hop tests
 *   t0_cv    the px entries with p > 0 and fl32(fl32(p+1)-1) >= theta_n (NULL: no >1-hop nodes -- modes "1-hop", "cn")
 *   u_cv     HASHED union of a node's adjacency row and its px row: row i owns u_buckets[i] buckets of 8 entries
 *            (64 aligned bytes, unused entries node INT32_MAX), entry (i, v) in bucket
 *            mulhi_u32(v * 2654435761 mod 2^32, u_buckets[i]), value = P[i, v] with the SIGN BIT set when v is
 *            adjacent to i; no bucket overflows (the builder grows a row's bucket count until that holds)
 *   mini     uint32 [n_nodes][32]: a fixed 1,024-bit absence filter of every union row -- key v sets bits h & 31 and
 *            (h >> 5) & 31 of word h >> 27, h = mix32(v ^ 0x9E3779B9) (graph.py mini_filters / bloom_hash).  The run
 *            kernel stages the filters of an item's endpoints in LDS and fetches a bucket only for candidates that
 *            pass: random reads are what bounds it (profiles/r04_random_read_probe.txt)
 * mode_cn: mask mode "cn" -- common neighbours only, round trip with t = 1, thresh_cn filter (:232-247).
 * use_px:  0 when theta_1 <= 0 (absent PPR entries then pass the one-hop test and px rows cannot stand in for them). */
int lpf_select3_plan(int64_t bs, const int64_t *batch, int64_t batch_ld, int64_t n_nodes, const void *node_rec,
                     const void *adj_cv, const void *a1_cv, const void *px_cv, const void *t0_cv, int32_t mode_cn,
                     int32_t use_px, void *desc, int64_t *offs, int32_t *item_pair, int64_t item_cap, int64_t *ctl,
                     uint64_t *plan_lb, void *stream);
int lpf_select3_run(int64_t bs, const void *desc, const int64_t *offs, const int32_t *item_pair, int64_t item_cap,
                    int64_t *ctl, uint64_t *run_lb, const void *u_cv, const void *mini, float th_cn, float th_1hop,
                    float th_non1hop, int32_t mode_cn, int32_t *type_ptr, void *entries, int64_t ent_cap,
                    int32_t grid_blocks, void *stream);

/* The same selection in ONE launch with PAIR-MAJOR output (select4.hip) -- the form the hot
 * path runs: compute_node_mask + get_ppr_vals + get_non_1hop_ppr (link_transformer.py:214-319,434-481) for the model's
 * own typing adjacency, same index arrays, same per-candidate arithmetic and therefore the same index sets and PPR
 * values bit for bit as lpf_select3_*.  A workgroup owns a block of LPF_SELECT4_BLOCK consecutive pairs: it plans their
 * walks itself (no plan launch, no descriptors in memory), types the block's candidate slots, and compacts the kept
 * entries in slot order -- a pair's entries are contiguous -- with ballot ranks and one scan inside the workgroup (no
 * chained scan over the batch).  Where a block lands in `entries` is one atomic add; consumers address entries through
 * pair_tab only, so results do not depend on it.
 *   entries   16-byte records {pair | type << 29 | from_N(b) << 31, node, pa, pb}, type 1 = common neighbour,
 *             2 = one-hop, 3 = >1-hop; a pair's entries in candidate-slot order (neighbours of a, then of b, then
 *             the >1-hop nodes), types mixed
 *   pair_tab  int32[bs][4] = {first entry, n_cn, n_1hop, n_non1hop} per pair
 *   blk_cnt   int32[ceil(bs / LPF_SELECT4_BLOCK)][2]: {selected entries, pairs with selected entries} per block of pairs;
 *             8-byte aligned (written and read as 8-byte pairs)
 *   ctl       int64[LPF_SELECT4_CTL_WORDS], zero-initialised once by the caller, then owned by the library (one control
 *             block per stream): [0] entries the last batch needed room for (the buffer is cut into 8 regions, workgroup
 *             g allocates its candidate slots -- rounded up to 8 -- in region g % 8: 8 x the fullest region -- an upper
 *             bound)  [1] the candidate slots of the last batch (every workgroup's rounded up to 8: the true sum over the
 *             regions)  [3] STICKY error bits as above  [10] completion counter, [16..23] allocation counters (zero
 *             between launches)
 * A block that does not fit below ent_cap leaves empty pairs and raises LPF_SELECT_ERR_ENTRY_CAP (consumers write NaN
 * rows while the bit is set).  threads: launch shape, workgroup size (256, 512 or 1024) + 4096 * (blocks of 64 pairs a workgroup
 * takes together - 1); 0 = the default (1024 threads; 2 blocks while that gives every CU a workgroup, else 1). */
#define LPF_SELECT4_BLOCK 64
#define LPF_SELECT4_CTL_WORDS 32
int lpf_select4(int64_t bs, const int64_t *batch, int64_t batch_ld, int64_t n_nodes, const void *node_rec,
                const void *adj_cv, const void *a1_cv, const void *px_cv, const void *t0_cv, const void *u_cv,
                const void *mini, int32_t mode_cn, int32_t use_px, float th_cn, float th_1hop, float th_non1hop,
                int64_t *ctl, void *pair_tab, int32_t *blk_cnt, void *blk_types, void *entries, int64_t ent_cap,
                int32_t threads, void *stream);

/* lpf_select4 that ALSO leaves the attention's per-pair query q_out[p, :q_dim] = q_tab[a_p] + q_tab[b_p] (that operand
 * order, = lpf_pair_gather_f32(sum) and lpf_dense_chain_side_f32; layers.py:212-215) for the pairs that KEPT at least one
 * entry -- the only pairs whose query lpf_pair_attention_rows4_* reads.  The rows of pairs without entries, and every row of
 * a workgroup that did not fit the entry buffer, are NOT written.  The workgroup that typed a block of pairs writes their
 * rows at its end, when the counts are final: no launch and no pass over memory for the other pairs' rows.
 *   q_tab  float [n_nodes, ld_q_tab] per-node table, q_out float [bs, ld_q_out]; q_dim % 4 == 0, q_dim <= 128, rows
 *          16-byte aligned.  q_out NULL: lpf_select4.
 * Added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays. */
int lpf_select4_q(int64_t bs, const int64_t *batch, int64_t batch_ld, int64_t n_nodes, const void *node_rec,
                  const void *adj_cv, const void *a1_cv, const void *px_cv, const void *t0_cv, const void *u_cv,
                  const void *mini, int32_t mode_cn, int32_t use_px, float th_cn, float th_1hop, float th_non1hop,
                  int64_t *ctl, void *pair_tab, int32_t *blk_cnt, void *blk_types, void *entries, int64_t ent_cap,
                  int32_t threads, const float *q_tab, int64_t ld_q_tab, float *q_out, int64_t ld_q_out, int32_t q_dim,
                  void *stream);

/* lpf_select4's result in the TYPE-MAJOR form of lpf_select3_run (what the matrix-core attention, the record-merging tail
 * and lpf_select_export read): type_ptr int32[3][bs + 1] per-type segment pointers and three regions of `ent_cap` 16-byte
 * records {pair | from_N(b) << 31, node, pa, pb} ordered by (pair, candidate slot) -- same sets, same values, same order
 * inside a pair's segment as lpf_select3_* leave.  For hub-heavy batches (ogbl-ppa-like: a pair's walks run to thousands
 * of candidate slots, a handful is kept) lpf_select4 + this launch cost the chip about half the CU-time of
 * lpf_select3_plan + _run: a block of 64 pairs keeps one workgroup busy for as long as ITS walks take instead of every
 * CU for as long as the batch's do.
 *   blk_types  int32[ceil(bs / LPF_SELECT4_BLOCK)][4] {common neighbours, one-hop, >1-hop, 0} kept per block: pass the
 *              same buffer to lpf_select4 (its optional blk_types argument; NULL there: not written)
 *   ctl        lpf_select4's control block; receives [4..6] the totals per type and the sticky LPF_SELECT_ERR_ENTRY_CAP
 *              when a region is too small (entries past ent_cap are dropped, type_ptr still counts them)
 * One wavefront per block: the per-pair pointers are an in-wave scan on top of the sum of the blocks in front, the
 * block's entries -- one contiguous run of the pair-major buffer -- move with ballot ranks. */
int lpf_select4_regions(int64_t bs, const void *pair_tab, const void *blk_types, const void *entries4, int64_t ent_cap4,
                        int32_t *type_ptr, void *regions, int64_t ent_cap, int64_t *ctl, void *stream);

/* The reference's layout from the regions above: all CN entries sorted by (pair, node), then all 1-hop (the two runs
 * merged by node id), then all >1-hop (link_transformer.py:161-162); type_ptr64 int64[3*(bs+1)] relative per type,
 * counts_f (optional) the float count features: n_counts = 4 -> get_structure_cnts (:340-356) n_cn, n_1hop,
 * n_non1hop, n_cn + n_1hop; 3 -> without n_non1hop (mask mode "1-hop"); 1 -> n_cn alone (mask mode "cn", :154-155). */
int lpf_select_export(int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap, int64_t *type_ptr64,
                      float *counts_f, int64_t ldc, int32_t n_counts, int32_t *sel_pair, int32_t *sel_node,
                      float *sel_pa, float *sel_pb, void *stream);

/* Attention scores for every selected entry (layers.py:206-218 with get_pos_encodings
 * link_transformer.py:182-211 folded in; algebra in DESIGN.md):
 *   h_e = ReLU(LN_t(W1_t [pa,pb] + b1_t)) + ReLU(LN_t(W1_t [pb,pa] + b1_t))
 *   k_e = Z[node_e] + Wfold_t h_e + bfold_t ;  score_e = sum_c att_c * leaky_relu(k_e,c * q[pair_e],c, 0.2)
 * Host-prepared, parameter-only tables (lpformer_amd/fold.py builds them in float64, stores fp32):
 *   pe_tab   float[3][D][4]  per type t and hidden unit k: (g_k (w0_k - mean w0), g_k (w1_k - mean w1),
 *                            g_k (b_k - mean b), beta_k) -- first PE Linear with the LayerNorm centring folded in
 *   pe_stat  float[6][8]     rows 0-2, per type: centred second moments over k of (w0, w1, b): C00, C11, Cbb, C01, C0b,
 *                            C1b, 0, c  (the LayerNorm variance of W1 [x,y] + b1 as a quadratic form in (x, y); the
 *                            statement of the form for host-side restatements, not read on the device);
 *                            rows 3-5, per type: l00, l10, l20, l11, l21, l22, 0, c: the lower-triangular factor L of
 *                            that moment matrix M = L L^T.  The kernels read these rows and take the variance as the
 *                            sum of squares (l00 x + l10 y + l20)^2 + (l11 y + l21)^2 + l22^2 (the quadratic form of M
 *                            written out cancels where w1 ~ -w0 and x ~ y); slot 7: the no-flip radius c of the
 *                            pair-major kernels (fold.no_flip_radius), unused elsewhere.
 *                            The table had rows 0-2 only before, which the kernels read; signatures are unchanged, and
 *                            the table is always made by fold.pe_tables of the package the library ships with.
 *   wfold_packed float[3][D/32][D/8][64][4]: element (t, c, sq, lane, u) = Wfold_t[32c + (lane&31)]
 *                            [(lane>>5)*(D/2) + 4 sq + u]  with Wfold_t = W_r[:, D:] W2_t  (MFMA A-operand order)
 *   bfold    float[3][D] = W_r[:, D:] (2 b2_t) ;  att float[D]
 * The number of entries is read from type_ptr on the device; max_entries (host-side capacity) only sizes the grid.
 * D in {32, 64, 128, 256}.  fp32 MFMA. */
int lpf_pair_scores_f32(int32_t D, const int64_t *type_ptr, int64_t bs, const int32_t *sel_pair,
                        const int32_t *sel_node, const float *sel_pa, const float *sel_pb,
                        const float *Z, int64_t ldz, const float *q, int64_t ldq,
                        const float *pe_tab, const float *pe_stat, const float *wfold_packed, const float *bfold,
                        const float *att, float *score, int64_t max_entries, void *stream);

/* Per-pair segment softmax (PyG softmax: max-shift, denominator + 1e-16; layers.py:220) and the weighted sums
 * that the output GEMM needs (layers.py:224 + scatter-sum):
 *   G[k, 0:D]   = sum_e alpha_e Z[node_e]
 *   G[k, (1+t)D : (2+t)D] = sum_{e of type t} alpha_e h_e          t = 0,1,2
 *   G[k, 4D + t] = sum_{e of type t} alpha_e ;  G[k, 4D+3] = 1
 * alpha_out (optional, NULL to skip): alpha per entry in the sel_* order (return_weights path, layers.py:73-75).
 * heavy_scratch: int32[bs+1] scratch (list of the pairs with many selected nodes, handled by a second kernel). */
int lpf_pair_softmax_gather_f32(int32_t D, int64_t bs, const int64_t *type_ptr, const int32_t *sel_node,
                                const float *sel_pa, const float *sel_pb, const float *score,
                                const float *Z, int64_t ldz, const float *pe_tab, const float *pe_stat,
                                float *G, int64_t ldg, float *alpha_out, int32_t *heavy_scratch, void *stream);

/* Per-pair attribution of the attention (csrc/explain.hip): the same PyG segment softmax over
 * a pair's CN, 1-hop and >1-hop entries JOINTLY (layers.py:220: max-shift, denominator + 1e-16) as
 * lpf_pair_softmax_gather_f32, reduced to what explains the pair instead of to the weighted sums -- the reference only
 * hands out (pair position, alpha) per entry (layers.py:73-75), without node ids or types.  Input: the layout of
 * lpf_select_export (type_ptr int64[3][bs+1] relative per type, sel_* type-major sorted by (pair, node)) and `score`
 * of lpf_pair_scores_f32.  Entry counts are read from type_ptr on the device; max_entries is the capacity of sel_*,
 * score and all_* (nothing is read or written past it).  Per pair p:
 *   mass     float[bs][3]   sum of alpha per type (CN, 1-hop, >1-hop); an empty pair: 0
 *   entropy  float[bs]      -sum alpha ln alpha in nats, terms with alpha = 0 contributing 0; an empty pair: 0
 *   top_*    [bs][top], 1 <= top <= 32: the entries with the largest alpha, best first, ties to the smaller node id, a
 *            NaN alpha last: top_node int64 (padding -1), top_w float (0), top_type int8 1 = CN, 2 = 1-hop, 3 = >1-hop
 *            (0), top_pa / top_pb float (0) the PPR values the positional encoding saw (link_transformer.py:182-211)
 *   all_*    optional (all_ptr NULL to skip) pair-major full list: all_ptr int64[bs+1] = the sum of the three type
 *            pointers, all_node int64 / all_type int8 / all_w float [max_entries]: a pair's entries in CN, 1-hop,
 *            >1-hop order, each sorted by node
 * heavy_scratch: int32[bs+1] (list of the pairs with many entries, taken by a whole workgroup in a second launch).
 * Sums are accumulated in fp64 and rounded once; no float atomics: results do not depend on the launch shape. */
int lpf_pair_explain_f32(int64_t bs, const int64_t *type_ptr, const int32_t *sel_node, const float *sel_pa,
                         const float *sel_pb, const float *score, int64_t max_entries, int32_t top, float *mass,
                         float *entropy, int64_t *top_node, float *top_w, int8_t *top_type, float *top_pa,
                         float *top_pb, int64_t *all_ptr, int64_t *all_node, int8_t *all_type, float *all_w,
                         int32_t *heavy_scratch, void *stream);

/* Fused dense chain (one launch):  y = L2( act( LN( L1(x) + addend ) ) )  on the fp32 matrix cores, hidden activations
 * never leaving registers.  Replaces Linear -> LayerNorm -> ReLU -> Linear chains of other_models.py:125-138 (MLP),
 * :173-179 (mlp_score, N2 == 1 "dot mode": logit/prob out), the hoisted lin_l of layers.py:212-215 (in_mode 2) and the
 * attention-output projection + post_att_norm (layers.py:78; single layer with addend + LN).
 *   in_mode 0: x = X[m, :K1]; 1: x = X[a_m] * X[b_m]; 2: x = X[a_m] + X[b_m]  (batch: int64 [2, M], row stride batch_ld;
 *              n_rows = rows of X, ids outside [0, n_rows) read row 0 -- see lpf_pair_gather_f32)
 *   w1_packed: layer-1 weights [N1, K1] in MFMA A-operand order, output tiles padded to an even count
 *              ntp1 = 2*ceil(N1/32).  k-group ks (16 input features) is ntp1*64 float4: float4 (c, lane = 16q + i) =
 *              W1[16c + i][16ks + 4q + 0..3].  A stage is one k-group, zero padded to a multiple of 512 float4; the
 *              image is the concatenation of ceil(K1 / 16) stages.
 *              b1, ln_g, ln_b: ntp1*16 floats, zero padded; ln_g NULL = no LayerNorm;
 *              flags & LPF_FLAG_RELU: ReLU after (the LayerNorm of) layer 1; addend [M, N1] optional (N1 % 4 == 0)
 *   w2_packed: NULL = single layer (out [M, N1]); N2 == 1: plain zero-padded vector of ntp1*16 floats, b2[0] the bias,
 *              out = logits [M] and/or prob = sigmoid [M]; otherwise [N2, N1] packed like w1 over the ntp1 hidden
 *              tiles as k-groups (ntp2 = 2*ceil(N2/32) output tiles); b2: ntp2*16 floats
 *   K1 % 4 == 0.  Built tile shapes (nt1, nt2): (2|3|4|5|8|9|16|17|32, 0), (2,2) (4,4) (8,8) (16,16), (3,2) (5,4) (9,8)
 *   (17,16); in_mode 1 for the square pairs and (2|4|8|16, 0), in_mode 2 for (2|4|8|16, 0);
 *   anything else returns LPF_ERR_UNSUPPORTED (callers then use lpf_gemm_f32 + lpf_layernorm_f32).
 *   lpformer_amd/fold.py builds the packed images. */
int lpf_dense_chain_f32(int64_t M, int32_t in_mode, const float *X, int64_t ldx, const int64_t *batch,
                        int64_t batch_ld, int64_t n_rows, int32_t K1, const float *w1_packed, int32_t N1, const float *b1,
                        const float *addend, int64_t ldadd, const float *ln_g, const float *ln_b, uint32_t flags,
                        const float *w2_packed, int32_t N2, const float *b2, float *out, int64_t ldo, float *prob,
                        void *stream);
/* lpf_dense_chain_f32 in a gather mode (in_mode 1 or 2) that ALSO leaves side_out[m, :side_dim] = S[a_m] + S[b_m] for a
 * second per-node table S [n_rows, ld_side_tab] read with the same ids -- lpf_pair_gather_f32 (sum) without a launch of
 * its own: the attention's per-pair query q = lin_l(x_a) + lin_l(x_b) from the table lin_l(X) (layers.py:212-215)
 * beside the elementwise branch of the same batch.  side_dim % 4 == 0, rows 16-byte aligned, a + b in that order. */
int lpf_dense_chain_side_f32(int64_t M, int32_t in_mode, const float *X, int64_t ldx, const int64_t *batch,
                             int64_t batch_ld, int64_t n_rows, int32_t K1, const float *w1_packed, int32_t N1,
                             const float *b1, const float *addend, int64_t ldadd, const float *ln_g, const float *ln_b,
                             uint32_t flags, const float *w2_packed, int32_t N2, const float *b2, float *out,
                             int64_t ldo, float *prob, const float *side_tab, int64_t ld_side_tab, int32_t side_dim,
                             float *side_out, int64_t ld_side_out, void *stream);

/* The dense tail of the scoring path in one launch (what LinkTransformer.score_pairs runs after the softmax-gather):
 *   o   = post_att_norm( G[:, D:] Wcat^T + G[:, :D] )                        (layers.py:78; G from
 *                                                                              lpf_pair_softmax_gather_f32)
 *   r_p = ReLU(LayerNorm( W_p0 [o | counts] + b_p0 ))                         first layer of pairwise_lin
 *   s   = w_dot . ReLU( W_C [r_e | r_p] + b_C ) + b_dot ;  prob = sigmoid(s)   score head, boundary Linears folded
 * D in {32, 64, 128} (else LPF_ERR_UNSUPPORTED: run the three lpf_dense_chain_f32 launches).  n_counts = 4 (3 in
 * "1-hop" mode; the fourth float of `counts` must then be 0).  Weight images in the lpf_dense_chain_f32 layout (one
 * k-group per stage): wA = Wcat [D, 3D+4]; wB = W_p0 [D+n, D+n]; wC = [A_e | A_p] laid out over D + 16*2*ceil((D+n)/32)
 * input columns (r_e first, then the even-tile-padded r_p).  lnA_*: D floats; bB, lnB_*: padded to the even tile
 * count of D+n; bC, w_dot: 2D floats; b_dot: 1 float.  r_e [M, D] = hidden activations of elementwise_lin. */
int lpf_tail_chain_f32(int64_t M, int32_t D, int32_t n_counts, const float *G, int64_t ldg, const float *wA_packed,
                       const float *lnA_g, const float *lnA_b, const float *counts, int64_t ldc,
                       const float *wB_packed, const float *bB, const float *lnB_g, const float *lnB_b,
                       const float *r_e, int64_t ldre, const float *wC_packed, const float *bC, const float *w_dot,
                       const float *b_dot, float *logit, float *prob, void *stream);

/* Attention in ONE pass over the regions written by lpf_select_run (pair_fused.hip): per entry
 *   k_e = Z[node] + Wfold_t h_e + bfold_t,  s_e = att . leaky_relu(k_e * q[pair], 0.2)        (layers.py:206-218)
 * then the segment softmax and the weighted sum (layers.py:220-224) as an online softmax per (pair, type) segment;
 * every Z row is gathered once, k_e and s_e never reach memory.  Output: for every non-empty segment
 *   part[(t*bs + pair)*(D+4) ..] = { sum_e exp(s_e - m) k_e [D], m = max_e s_e, l = sum_e exp(s_e - m), -, - }
 * A segment that crosses 16-entry unit boundaries of its type's region leaves instead one boundary record per unit it
 * touches: bnd[((t*units_cap + U)*2 + slot)*(D+4) ..], slot 1 of the unit it starts in, slot 0 of every following
 * unit.  lpf_tail_chain_merge_f32 combines a pair's records (it finds the boundary records from the segment
 * pointers).  Tables as for lpf_pair_scores_f32.
 * bnd: float[3*units_cap*2*(D+4)], units_cap >= ceil(ent_cap/16).  D in {32, 64, 128}. */
int lpf_pair_attention_fused_f32(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries,
                                 int64_t ent_cap, const float *Z, int64_t ldz, const float *q, int64_t ldq,
                                 const float *pe_tab, const float *pe_stat, const float *wfold_packed,
                                 const float *bfold, const float *att, float *part, float *bnd,
                                 int64_t units_cap, void *stream);

/* bf16 THROUGHPUT MODE of lpf_pair_attention_fused_f32 (BASELINE.json config 2 names bf16 storage): the node table
 * Z is stored in bf16 (half the gather bytes: rows of 2 D bytes staged by LDS-DMA) and Wfold_t h_e runs on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; h_e is generated in fp32 and rounded to bf16 as the A operand.
 * Everything else (q, bfold, att, scores, softmax, records) stays fp32, and the selection never touches bf16, so the
 * selected index sets are unchanged.  Logits differ from the fp32 path by the bf16 rounding of Z and Wfold (tests state
 * the tolerance).
 *   Z_bf16            bf16 [N, ldz] (ldz in elements, rows 16-byte aligned)
 *   wfold_packed_bf16 bf16 [3][D/32][D/16][64][8]: element (t, c, s, lane, j) =
 *                     Wfold_t[32 c + (lane & 31)][16 s + 8 (lane >> 5) + j]   (MFMA B-operand order) */
int lpf_pair_attention_fused_bf16(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries,
                                  int64_t ent_cap, const void *Z_bf16, int64_t ldz, const float *q, int64_t ldq,
                                  const float *pe_tab, const float *pe_stat, const void *wfold_packed_bf16,
                                  const float *bfold, const float *att, float *part, float *bnd,
                                  int64_t units_cap, void *stream);

/* One-pass attention WITHOUT the D x D product per entry (pair_flip.hip): same inputs, records and consumers as
 * lpf_pair_attention_fused_f32, fp32 throughout.  The hidden layer of the PE MLP is affine in (r pa, r pb, r, 1) on
 * every set of active units, so with the four D-vectors of the units active at (0, 0) precomputed
 *   Wfold_t h_e + bfold_t = P0 (r1 pa + r2 pb) + Q0 (r1 pb + r2 pa) + R0 (r1 + r2) + C0 + sum_{k flipped} Wfold_t[:,k] |y_k|
 * (exact for every input; a unit is "flipped" when its ReLU state differs from the one at (0, 0)).  Tables from
 * lpformer_amd/fold.py flip_tables: pe_tab_signed float[3][D][4] = the pe_tab row of a unit times +1 when the unit is
 * active at (0, 0) and -1 when it is not (the kernel then sees a flipped unit as a NEGATIVE pre-activation of
 * magnitude |y_k|), base float[3][4][D] = (P0, Q0, R0, C0), wfold_t float[3][D][D] (wfold_t[t][k][c] = Wfold_t[c][k]).
 * Bound: vector-ALU issue (about ninety instructions per entry plus a dozen per flipped unit); the Z-row gather
 * (4 D + 16 bytes per entry) hides under it. */
int lpf_pair_attention_flip_f32(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap,
                                const float *Z, int64_t ldz, const float *q, int64_t ldq, const float *pe_tab_signed,
                                const float *pe_stat, const float *base, const float *wfold_t, const float *att,
                                float *part, float *bnd, int64_t units_cap, void *stream);

/* The same with the node table Z stored in bf16 (Z_bf16: uint16 rows, ldz in elements, a multiple of 8): the attention
 * kernel of the bf16 throughput mode for D >= 128.  Z is widened to fp32 on arrival; q, tables, arithmetic and records
 * are those of lpf_pair_attention_flip_f32. */
int lpf_pair_attention_flip_zbf16(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap,
                                  const void *Z_bf16, int64_t ldz, const float *q, int64_t ldq,
                                  const float *pe_tab_signed, const float *pe_stat, const float *base,
                                  const float *wfold_t, const float *att, float *part, float *bnd, int64_t units_cap,
                                  void *stream);

/* The attention OUTPUT of every pair from the records of lpf_pair_attention_fused_f32 (for callers that want
 * features, calc_pairwise link_transformer.py:132-178, rather than scores):
 *   out[p, :D] = post_att_norm( merged record of pair p + att_bias )   (layers.py:78,220; PyG softmax, +1e-16 once)
 *   out[p, D..] = n_cn, n_1hop, [n_non1hop,] n_cn + n_1hop             (get_structure_cnts, link_transformer.py:340-356)
 * ldo >= D + n_counts, ldo % 4 == 0.  Rows are NaN when sel_ctl[3] != 0 (selection workspace overflow). */
int lpf_pair_attention_merge_f32(int64_t bs, int32_t D, int32_t n_counts, const float *part, const float *bnd,
                                 int64_t units_cap, const int32_t *type_ptr, const float *att_bias, const float *ln_g,
                                 const float *ln_b, const int64_t *sel_ctl, float *out, int64_t ldo, void *stream);

/* lpf_tail_chain_f32 with the attention output taken from the records of lpf_pair_attention_fused_f32 instead of a
 * GEMM:  o = post_att_norm( sum_t e^{m_t-M} acc_t / (sum_t e^{m_t-M} l_t + 1e-16) + att_bias ), M = max_t m_t over the
 * pair's non-empty segments (PyG softmax over ALL entries of the pair, layers.py:220; no entry => o = LN(att_bias)),
 * and the count features n_cn, n_1hop, [n_non1hop,] n_cn+n_1hop (link_transformer.py:340-356) from type_ptr.
 * sel_ctl (optional): the selection control block; if its error word is set every score of the batch is NaN. */
int lpf_tail_chain_merge_f32(int64_t M, int32_t D, int32_t n_counts, const float *part, const float *bnd,
                             int64_t units_cap, const int32_t *type_ptr, const float *att_bias, const float *lnA_g, const float *lnA_b, const float *wB_packed,
                             const float *bB, const float *lnB_g, const float *lnB_b, const float *r_e, int64_t ldre,
                             const float *wC_packed, const float *bC, const float *w_dot, const float *b_dot,
                             const int64_t *sel_ctl, float *logit, float *prob, void *stream);
/* bf16 THROUGHPUT MODE of the dense tail (SURVEY 8b lpf_pair_head_bf16): the two GEMMs run on
 * v_mfma_f32_16x16x16_bf16 -- weights wB / wC as bf16 images in the same element order as the fp32 ones (a lane's four
 * consecutive fp32 become its four bf16), activations rounded to bf16 as they enter a GEMM, fp32 accumulate; the
 * record merge, both LayerNorms, the dot product and the sigmoid stay fp32. */
int lpf_tail_chain_merge_bf16(int64_t M, int32_t D, int32_t n_counts, const float *part, const float *bnd,
                             int64_t units_cap, const int32_t *type_ptr, const float *att_bias, const float *lnA_g, const float *lnA_b, const void *wB_packed_bf16,
                             const float *bB, const float *lnB_g, const float *lnB_b, const float *r_e, int64_t ldre,
                             const void *wC_packed_bf16, const float *bC, const float *w_dot, const float *b_dot,
                             const int64_t *sel_ctl, float *logit, float *prob, void *stream);

/* One-pass attention PAIR-MAJOR (pair_rows.hip; replaces lpf_pair_attention_flip_* + the record merge on the hot path):
 * LinkAttention.message + PyG softmax + scatter-sum + LinkAttention.bias + post_att_norm (src/modules/layers.py:66-78,
 * 193-224) and get_structure_cnts (src/models/link_transformer.py:340-356), with the positional encodings
 * (link_transformer.py:182-211) folded in as in lpf_pair_attention_flip_f32 (same tables).  A group of D/4 lanes walks
 * the entries PAIR-MAJOR -- a pair's three segments one after the other, found from type_ptr, 16 consecutive entries
 * per work unit -- and the kernel writes every pair's finished row once:
 *   out[p, :D]  = post_att_norm( sum_e alpha_e k_e + att_bias )          (no entry: post_att_norm(att_bias))
 *   out[p, D..] = n_cn, n_1hop, [n_non1hop,] n_cn + n_1hop               (n_counts of them; n_counts = 0: none written)
 * A pair inside one unit is finished in registers; one that crosses units leaves a partial state per unit in `pieces`,
 * merged in unit order by the workgroup that owns the pair before the launch ends: nothing is left for the consumer.
 * ldo >= D + n_counts, ldo % 4 == 0.  Rows are NaN when sel_ctl[3] != 0 (selection workspace overflow).
 * pieces: scratch, float[units_cap * 2 * lpf_pair_rows_piece_floats(D)], units_cap >= ceil(3 * ent_cap / 16) + 1 -- the
 * partial softmax states of the pairs that cross the 16-entry units of the pair-major order (written and merged inside
 * the launch, by the workgroup that owns the pair; contents are meaningless afterwards).  D in {32, 64, 128, 256}. */
int lpf_pair_attention_rows_f32(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap,
                                const float *Z, int64_t ldz, const float *q, int64_t ldq, const float *pe_tab_signed,
                                const float *pe_stat, const float *base, const float *wfold_t, const float *att,
                                const float *att_bias, const float *ln_g, const float *ln_b, int32_t n_counts,
                                const int64_t *sel_ctl, float *pieces, int64_t units_cap, float *out, int64_t ldo,
                                void *stream);
int64_t lpf_pair_rows_piece_floats(int32_t D);
/* The same with the node table Z stored in bf16 (uint16 rows, ldz in elements, a multiple of 8). */
int lpf_pair_attention_rows_zbf16(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap,
                                  const void *Z_bf16, int64_t ldz, const float *q, int64_t ldq,
                                  const float *pe_tab_signed, const float *pe_stat, const float *base,
                                  const float *wfold_t, const float *att, const float *att_bias, const float *ln_g,
                                  const float *ln_b, int32_t n_counts, const int64_t *sel_ctl, float *pieces,
                                  int64_t units_cap, float *out, int64_t ldo, void *stream);

/* lpf_tail_chain_f32 behind lpf_pair_attention_rows_*: stage A is a plain read of the pair's finished row
 * rows[p] = [post_att_norm(attention output) (D) | count features, zero padded to 4] (ldrows >= D + 4); what is left is
 * the first layer of pairwise_lin, its LayerNorm + ReLU, the folded score head and the sigmoid
 * (other_models.py:80-179, link_transformer.py:170-177).  sel_ctl as for lpf_tail_chain_merge_f32.  D in {32, 64, 128}. */
int lpf_tail_chain_rows_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                            const float *wB_packed, const float *bB, const float *lnB_g, const float *lnB_b,
                            const float *r_e, int64_t ldre, const float *wC_packed, const float *bC, const float *w_dot,
                            const float *b_dot, const int64_t *sel_ctl, float *logit, float *prob, void *stream);
/* ... with bf16 weights and v_mfma_f32_16x16x16_bf16 for the two GEMMs (as lpf_tail_chain_merge_bf16). */
int lpf_tail_chain_rows_bf16(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                             const void *wB_packed_bf16, const float *bB, const float *lnB_g, const float *lnB_b,
                             const float *r_e, int64_t ldre, const void *wC_packed_bf16, const float *bC,
                             const float *w_dot, const float *b_dot, const int64_t *sel_ctl, float *logit, float *prob,
                             void *stream);

/* The pair of launches with the pairs WITHOUT selected nodes handled apart.  Such a pair's attention branch is a constant
 * -- softmax over nothing, so the row is post_att_norm(att_bias) with zero counts (layers.py:66-78,
 * link_transformer.py:340-356) -- and so is everything pairwise_lin makes of it: its score needs the elementwise half of
 * the folded head only.  lpf_pair_attention_rows_perm_* additionally leaves the ORDER the tail walks the pairs in:
 *   perm int32[bs]: the pairs with selected nodes in ascending order, then -- from the back, descending towards the
 *                   front -- the ones without;  *n_nonempty: how many have selected nodes.  (Deterministic: a chained scan
 *                   over the workgroups, no atomics on a counter.)
 *   perm_lb uint64[LPF_ROWS_PERM_LB_WORDS]: the scan's words; zero before the first launch, then left alone (the
 *                   kernel tags them with a launch number it keeps in the last word).  One buffer per stream.
 * lpf_tail_chain_rows_perm_* walks the pairs in that order; a workgroup whose 64 pairs all lie behind *n_full computes
 *   score = w_dot . ReLU(A_e r_e + bC_empty) + b_dot,    bC_empty [2 D] = bC + A_p r_p0
 * with r_p0 the hidden activation of pairwise_lin for the constant row (lpformer_amd/fold.py empty_pair_head_bias); every
 * other workgroup runs the full tail.  In a MIXED workgroup a pair without selected nodes takes its row from row_empty
 * [D] = post_att_norm(att_bias) (lpformer_amd/fold.py empty_pair_row) and zero counts; row_empty NULL: it reads rows[] like
 * any other pair (lpf_pair_attention_rows_perm_* writes the constant row there; lpf_pair_attention_rows4_* with an order
 * does NOT write rows or counts of such pairs: pass row_empty behind it).  Outputs are indexed by pair as before. */
#define LPF_ROWS_PERM_LB_WORDS 1025
int lpf_pair_attention_rows_perm_f32(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries, int64_t ent_cap,
                                     const float *Z, int64_t ldz, const float *q, int64_t ldq,
                                     const float *pe_tab_signed, const float *pe_stat, const float *base,
                                     const float *wfold_t, const float *att, const float *att_bias, const float *ln_g,
                                     const float *ln_b, int32_t n_counts, const int64_t *sel_ctl, float *pieces,
                                     int64_t units_cap, float *out, int64_t ldo, int32_t *perm, uint64_t *perm_lb,
                                     int64_t *n_nonempty, void *stream);
int lpf_pair_attention_rows_perm_zbf16(int32_t D, int64_t bs, const int32_t *type_ptr, const void *entries,
                                       int64_t ent_cap, const void *Z_bf16, int64_t ldz, const float *q, int64_t ldq,
                                       const float *pe_tab_signed, const float *pe_stat, const float *base,
                                       const float *wfold_t, const float *att, const float *att_bias,
                                       const float *ln_g, const float *ln_b, int32_t n_counts, const int64_t *sel_ctl,
                                       float *pieces, int64_t units_cap, float *out, int64_t ldo, int32_t *perm,
                                       uint64_t *perm_lb, int64_t *n_nonempty, void *stream);
/* lpf_pair_attention_rows_perm_* behind lpf_select4: the entries are pair-major already (a pair's entries contiguous from
 * pair_tab[p][0], the type in bits 29-30 of the record's pair word), so the kernel reads ONE region and needs no per-type
 * pointers; its workgroups split the batch by blk_cnt (entries per LPF_SELECT4_BLOCK pairs) and the 64 table entries of the
 * block a cut falls into.  units_cap: 16-entry units the `pieces` scratch has room for -- it bounds the SELECTED entries
 * of a batch (16 * (units_cap - 1)), not the entry buffer; a batch with more leaves NaN rows and raises
 * LPF_SELECT_ERR_ENTRY_CAP in sel_ctl[3].  perm / n_nonempty: both, or both NULL (no order for the
 * tail; the order needs no scan words here: the selection counted the pairs with entries per block; WITH an order the
 * rows and count features of pairs without entries are not written -- lpf_tail_chain_rows_perm_* takes row_empty for
 * them).
 * ACTIVATION PATTERNS BY TABLE (link_transformer.py:67-76,182-211 -- the PE MLPs' hidden ReLU -- layers.py:193-224): the
 * type-major calls know the base vectors of ONE activation pattern of the PE hidden layer, the one of (pa, pb) = (0, 0),
 * and pay per entry for finding and correcting the units that left it (`base`, `wfold_t`).  Here the plane of PPR value
 * pairs is cut into grid_n x grid_n cells, cell(v) = clamp((bits(fp32(v + grid_ofs)) >> grid_shift) - grid_base, 0,
 * grid_n - 1) on either axis, and
 *   pat_grid uint8 [3][grid_n][grid_n]: per type, cell (cell(x), cell(y)) -> bits 0-4: id s < LPF_ROWS_PATTERNS of a
 *       tabulated pattern, bit 7 clear: s is the pattern of EVERY point (x, y) of the cell; bit 7 set (a boundary may
 *       cross the cell, or its pattern is not tabulated): s is the tabulated pattern nearest to the pattern of the cell's
 *       centre, and the entry takes the exact path -- the units whose state differs from pattern s are found
 *       (pe_tab_signed, signed for pattern 0, with pat_sign) and corrected (wfold_t) one by one; the last cell of either
 *       axis (values > 1, NaN, negative) must be 0x80;
 *   pat_base float [3][LPF_ROWS_PATTERNS][4][D]: (P_s, Q_s, R_s, B_s + bfold / 2) with X_s = sum over the units k active
 *       in pattern s of Wfold[:, k] * (ta_k, tc_k, td_k, beta_k); id 0 = the pattern of (0, 0);
 *   pat_sign uint32 [3][LPF_ROWS_PATTERNS][D / 32]: bit k of pattern s = unit k is active in exactly one of pattern s and
 *       pattern 0.
 * An entry's key is Z[v] + [P r1 pa + Q r1 pb + R r1 + B](pattern of (pa, pb)) + [P r2 pb + Q r2 pa + R r2 + B](pattern
 * of (pb, pa)): no look at its 2 D units at all.  Built by lpformer_amd/patterns.py (a per-cell proof by convexity;
 * which patterns are tabulated only decides how many entries take the slower path, never a result).  A kernel that
 * cannot hold LPF_ROWS_PATTERNS patterns per type in LDS (D = 256) keeps the first half and treats higher ids as 0x80.
 * Everything else as lpf_pair_attention_rows_f32; the rows agree with that call's up to rounding (the order in which a
 * pair's entries are summed, the association of the base vectors). */
#define LPF_ROWS_PATTERNS 16
int lpf_pair_attention_rows4_f32(int32_t D, int64_t bs, const void *pair_tab, const int32_t *blk_cnt, const void *entries,
                                 int64_t ent_cap, const float *Z, int64_t ldz, const float *q, int64_t ldq,
                                 const float *pe_tab_signed, const float *pe_stat, const float *pat_base,
                                 const void *pat_grid, const void *pat_sign, int32_t grid_n, int32_t grid_shift,
                                 int32_t grid_base, float grid_ofs, const float *wfold_t, const float *att, const float *att_bias,
                                 const float *ln_g, const float *ln_b, int32_t n_counts, const int64_t *sel_ctl,
                                 float *pieces, int64_t units_cap, float *out, int64_t ldo, int32_t *perm,
                                 int64_t *n_nonempty, void *stream);
int lpf_pair_attention_rows4_zbf16(int32_t D, int64_t bs, const void *pair_tab, const int32_t *blk_cnt,
                                   const void *entries, int64_t ent_cap, const void *Z_bf16, int64_t ldz, const float *q,
                                   int64_t ldq, const float *pe_tab_signed, const float *pe_stat, const float *pat_base,
                                   const void *pat_grid, const void *pat_sign, int32_t grid_n, int32_t grid_shift,
                                   int32_t grid_base, float grid_ofs, const float *wfold_t, const float *att, const float *att_bias,
                                   const float *ln_g, const float *ln_b, int32_t n_counts, const int64_t *sel_ctl,
                                   float *pieces, int64_t units_cap, float *out, int64_t ldo, int32_t *perm,
                                   int64_t *n_nonempty, void *stream);

/* The dense tail behind that order (perm / n_full / bC_empty / row_empty: the paragraph in front of
 * lpf_pair_attention_rows_perm_f32; other_models.py:80-179, link_transformer.py:101-105,170-177). */
int lpf_tail_chain_rows_perm_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                 const float *wB_packed, const float *bB, const float *lnB_g, const float *lnB_b,
                                 const float *r_e, int64_t ldre, const float *wC_packed, const float *bC,
                                 const float *w_dot, const float *b_dot, const int64_t *sel_ctl, const int32_t *perm,
                                 const int64_t *n_full, const float *bC_empty, const float *row_empty, float *logit,
                                 float *prob, void *stream);
int lpf_tail_chain_rows_perm_bf16(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                  const void *wB_packed_bf16, const float *bB, const float *lnB_g, const float *lnB_b,
                                  const float *r_e, int64_t ldre, const void *wC_packed_bf16, const float *bC,
                                  const float *w_dot, const float *b_dot, const int64_t *sel_ctl, const int32_t *perm,
                                  const int64_t *n_full, const float *bC_empty, const float *row_empty, float *logit,
                                  float *prob, void *stream);
/* lpf_tail_chain_rows_perm_f32 that computes r_e itself: r_e[m] = ReLU(LayerNorm(W_e0 (X[a_m] * X[b_m]) + b_e0)), the
 * first layer of elementwise_lin (other_models.py:125-138), is a stage of the tail's own workgroups ("stage E": the gather
 * and arithmetic of lpf_dense_chain_f32 with in_mode 1, operation for operation), handed to the score head through LDS --
 * no r_e buffer, no launch of the elementwise branch.  The scores are bitwise those of lpf_dense_chain_f32 (-> r_e) +
 * lpf_tail_chain_rows_perm_f32.
 *   X float [n_rows, ldx] node table, batch int64 [2][batch_ld] (ids outside [0, n_rows) read row 0), wE_packed the packed
 *   image of W_e0 [D, D] (fold.dense_chain_tables: w1p), bE / lnE_g / lnE_b float [D].
 * wE_packed NULL: r_e is read from memory, exactly lpf_tail_chain_rows_perm_f32 (X, batch and the E tables are then
 * ignored).  With wE_packed, r_e is ignored.  Built for D = 128; other widths return LPF_ERR_UNSUPPORTED.
 * Added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays. */
int lpf_tail_chain_rows_perm_ew_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                    const float *wB_packed, const float *bB, const float *lnB_g, const float *lnB_b,
                                    const float *r_e, int64_t ldre, const float *wC_packed, const float *bC,
                                    const float *w_dot, const float *b_dot, const int64_t *sel_ctl, const int32_t *perm,
                                    const int64_t *n_full, const float *bC_empty, const float *row_empty,
                                    const float *X, int64_t ldx, const int64_t *batch, int64_t batch_ld, int64_t n_rows,
                                    const float *wE_packed, const float *bE, const float *lnE_g, const float *lnE_b,
                                    float *logit, float *prob, void *stream);

/* logit[i] = dot(A[i,:], w) + b ; prob[i] = sigmoid(logit[i])  (mlp_score last layer, other_models.py:178-179).
 * logit or prob may be NULL. */
int lpf_rowdot_sigmoid_f32(int64_t M, int32_t K, const float *A, int64_t lda, const float *w, float b,
                           float *logit, float *prob, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side PPR producer: the same Andersen push as lpf_ppr_push_cpu below, on the GPU.
 * calc_ppr (src/util/calc_ppr_scores.py:136-192) + create_sparse_ppr_matrix (:221-241): LIFO stack and float64
 * arithmetic per source in the reference's order, so index sets and fp32 values are bit-identical.  One wavefront
 * per source (dynamic assignment), neighbours of a popped node across the lanes; every wavefront owns dense
 * epoch-stamped state over all n nodes (32 n bytes) inside `workspace`.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of `workspace` for n_waves concurrent sources (n_waves: multiple of 4; 4096-8192 fills an MI355X). */
int64_t lpf_ppr_push_workspace_bytes(int64_t n, int64_t n_waves, double alpha, double eps);

/* rowptr/col: CSR of the coalesced directed edge list (get_ppr_matrix, :111-117), device memory.
 * Row i of the result lands UNSORTED at pool_col/pool_val[row_off[i] .. row_off[i] + row_len[i]) (rows are placed in
 * completion order).  counters int64[4] on return: [1] = total entries (if > pool_capacity nothing was written for
 * the rows that did not fit: call again with a pool of that size), [2] = rows that overflowed their
 * 1/(alpha*eps) list bound (must be 0). */
int lpf_ppr_push_f64(int64_t n, const int64_t *rowptr, const int32_t *col, double alpha, double eps,
                     int64_t n_waves, void *workspace, int64_t workspace_bytes, int32_t *pool_col, float *pool_val,
                     int64_t pool_capacity, int64_t *row_off, int32_t *row_len, int64_t *counters, void *stream);

/* The same push for the sources `sources[0 .. n_src)` only (device memory, ids in [0, n), STRICTLY ASCENDING: the dense
 * state is stamped with the source id).  row_off / row_len are indexed by LIST POSITION (n_src entries); everything
 * else as lpf_ppr_push_f64, with which it shares the kernel body.  Size n_waves by the list, not by n: the state that
 * is cleared per call is 32 n bytes per wavefront. */
int lpf_ppr_push_f64_sources(int64_t n, const int64_t *rowptr, const int32_t *col, int64_t n_src,
                             const int32_t *sources, double alpha, double eps, int64_t n_waves, void *workspace,
                             int64_t workspace_bytes, int32_t *pool_col, float *pool_val, int64_t pool_capacity,
                             int64_t *row_off, int32_t *row_len, int64_t *counters, void *stream);

/* Sort every row by column and pack the CSR (out_rowptr int64[n+1], out_col/out_val [nnz], nnz = counters[1] above). */
int64_t lpf_ppr_pack_workspace_bytes(int64_t n, int64_t nnz);
int lpf_ppr_pack_csr(int64_t n, const int64_t *row_off, const int32_t *row_len, const int32_t *pool_col,
                     const float *pool_val, int64_t nnz, int64_t *out_rowptr, int32_t *out_col, float *out_val,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Incremental refresh of the PPR matrix after a graph edit (csrc/ppr_update.hip; lpformer_amd/graph_update.py).
 * A row of the matrix holds every node its push popped, so a row without any KEY node (endpoints of added / removed
 * edges, old neighbours of removal endpoints) is bit-identical on the edited graph: only the other rows are pushed
 * again (lpf_ppr_push_f64_sources) and spliced into the old CSR.
 * ---------------------------------------------------------------------------------------------- */

/* flag[i] = 1 when row i of the CSR (rowptr int64[n+1], col int32) holds a node whose bit is set in key_bitmap
 * (uint32[(n + 31) / 32], node v = bit v & 31 of word v >> 5), else 0; list = the flagged row ids ascending (room for
 * n), *count = how many (device memory; nothing is read back).  bitmap_mode: 1 = every workgroup stages the bitmap in
 * LDS (n <= 524,288), 0 = probes in global memory, -1 = LDS up to 40 KiB of bitmap. */
int64_t lpf_ppr_affected_workspace_bytes(int64_t n);
int lpf_ppr_affected_rows(int64_t n, const int64_t *rowptr, const int32_t *col, const uint32_t *key_bitmap,
                          int32_t bitmap_mode, int32_t *flag, int32_t *list, int64_t *count, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* New CSR from the old one and the re-pushed rows of `sources[0 .. n_src)` (distinct ids; row_off / row_len / pool_* as
 * lpf_ppr_push_f64_sources left them, nnz_pool = its counters[1]): row i is the old row, or, for a listed source, its
 * new row sorted by column.  out_capacity = entries out_col / out_val have room for; the caller sizes it as
 * old nnz - (old lengths of the listed rows) + nnz_pool, rows that would pass it are not written. */
int64_t lpf_ppr_splice_workspace_bytes(int64_t n, int64_t n_src, int64_t nnz_pool);
int lpf_ppr_splice_csr(int64_t n, const int64_t *old_rowptr, const int32_t *old_col, const float *old_val,
                       int64_t n_src, const int32_t *sources, const int64_t *row_off, const int32_t *row_len,
                       const int32_t *pool_col, const float *pool_val, int64_t nnz_pool, int64_t *out_rowptr,
                       int32_t *out_col, float *out_val, int64_t out_capacity, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Per-model indexes over the PPR matrix, built on the device.  Selection results are identical
 * with and without them.
 *   mode 0: the >1-hop candidates  p > 0 and fl32(fl32(p+1)-1) >= theta   (link_transformer.py:464-478)  -> "T0"
 *   mode 1: the one-hop candidates fl32(fl32(p+1)-1) >= theta             (link_transformer.py:241-250,290-317) -> "P1"
 * Two steps around an exclusive scan of out_len by the caller: count per row, then fill (column order preserved).
 * ---------------------------------------------------------------------------------------------- */
int lpf_ppr_filter_count(int64_t n, const int64_t *rowptr, const float *val, int32_t mode, float theta,
                         int64_t *out_len, void *stream);
int lpf_ppr_filter_fill(int64_t n, const int64_t *rowptr, const int32_t *col, const float *val, int32_t mode,
                        float theta, const int64_t *out_rowptr, int32_t *out_col, float *out_val, void *stream);

/* selfp[e] = P[i, j] for every adjacency entry e = (i, j) (0 where the PPR matrix stores nothing): the PPR of a node
 * to its own neighbours, aligned with the adjacency CSR (the adj_selfp argument of lpf_select_run). */
int lpf_self_ppr(int64_t n, const int64_t *adj_rowptr, const int32_t *adj_col, const int64_t *ppr_rowptr,
                 const int32_t *ppr_col, const float *ppr_val, float *selfp, void *stream);

/* out[q] = M[rows[q], cols[q]] of a CSR matrix with sorted int32 columns (0 where nothing is stored or an id lies outside
 * [0, n)).  Used for the raw PPR values of the few selected entries whose TYPE changes when the training loop removes
 * the batch's positive edges from the typing adjacency (src/train/train_model.py:40-46; a common neighbour of (a, b)
 * that loses its edge to a becomes a one-hop node and its values are the other type's round trip of the raw value,
 * src/models/link_transformer.py:229-237,290-291): lpformer_amd.LinkTransformer._patch_removed. */
int lpf_csr_lookup_f32(int64_t nq, int64_t n, const int64_t *rows, const int64_t *cols, const int64_t *rowptr,
                       const int32_t *col, const float *val, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pair heuristics (pair_heuristics.hip): common neighbours, Adamic-Adar, Resource Allocation of candidate pairs on a
 * binary CSR -- the typing adjacency.  Replaces compute_edge_cn (src/train/eval.py:21-41: (A[a] & A[b]).sum() over
 * dense adj[edge].to_dense() rows per batch), which test_by_metric (eval.py:44-77) bins the test positives by, the
 * analysis behind run.py's --bymetric / --percentile arguments (src/run.py:195-196, parsed and never read there).
 * ---------------------------------------------------------------------------------------------- */
/* Walked rows longer than this go to the workgroup-per-pair kernel (split_threshold < 0 selects it). */
#define LPF_HEUR_SPLIT_DEFAULT 32
/* For pair p = (a, b) = (pairs[p], pairs[pairs_ld + p]) of a CSR with sorted, unique columns (values ignored):
 *   cn[p] = |N(a) & N(b)| (deg(a) when a == b; a stored self-loop counts like any other column),
 *   aa[p] = sum over w in N(a) & N(b) of w_aa[w],  ra[p] = the same sum of w_ra[w]
 * (w_aa[w] = 1 / ln deg(w), 0 where deg <= 1; w_ra[w] = 1 / deg(w): float[n] tables built once per graph).
 * Ids outside [0, n) give 0 / 0 / 0.  cn / aa / ra may each be NULL (not computed); w_aa / w_ra may be NULL when aa /
 * ra is.  A pair walks its shorter row (equal lengths: the row of min(a, b)) and binary-searches the other: pairs whose
 * walked row holds at most split_threshold entries are flattened 64 probes per wavefront, longer ones get a 256-thread
 * workgroup each (a second kernel over a list the first one fills).  Sums are fp64 in an order fixed by the pair
 * alone, rounded to fp32 once: h(a, b) and h(b, a) are bitwise equal, and so are two runs.
 * scratch: int32[P + 1] (the long-pair list).  P < 2^31 - 1. */
int lpf_pair_heuristics_f32(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                            const int32_t *col, const float *w_aa, const float *w_ra, int32_t split_threshold,
                            int32_t *scratch, int32_t *cn, float *aa, float *ra, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Top-K link recommendation (recommend.hip): the candidate pairs of a batch of sources and the segmented top-K of
 * their scores.  The reference only ranks a positive against negatives it is handed (src/train/testing.py:14-121).
 * ---------------------------------------------------------------------------------------------- */
/* Include rows longer than this go to the workgroup-per-source kernel (split_threshold < 0 selects it). */
#define LPF_REC_SPLIT_DEFAULT 256
/* Candidates of source u = sources[s]: the entries v of u's row of the include CSR (inc_*, fp32 values) whose value is
 * > 0 and >= min_val -- or every v of [0, n) when inc_rowptr is NULL -- minus u's row of the exclusion CSR (exc_*,
 * values ignored; NULL: none) and, with exclude_self, minus u; ascending v.  Sources outside [0, n) have none.
 * Count pass: count[s] = the number of candidates.  Fill pass: offset[s] = the exclusive scan of the counts of this
 * same call (P = their total); writes pairs[offset[s] + r] = u, pairs[P + offset[s] + r] = v_r (the [2, P] int64 layout
 * of the scoring sweep).  Include rows of at most split_threshold entries take one wavefront per source (exclusion
 * row staged in LDS when short, ranks by ballot); longer rows, and every row when inc_rowptr is NULL, get a 256-thread
 * workgroup each from a second kernel over a list the first fills.  scratch: int32[S + 1].  S, n < 2^31. */
int lpf_rec_candidate_count(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr,
                            const int32_t *inc_col, const float *inc_val, float min_val, const int64_t *exc_rowptr,
                            const int32_t *exc_col, int32_t exclude_self, int32_t split_threshold, int32_t *scratch,
                            int64_t *count, void *stream);
int lpf_rec_candidate_fill(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr,
                           const int32_t *inc_col, const float *inc_val, float min_val, const int64_t *exc_rowptr,
                           const int32_t *exc_col, int32_t exclude_self, int32_t split_threshold, int32_t *scratch,
                           const int64_t *offset, int64_t P, int64_t *pairs, void *stream);
/* Largest k of the segmented top-K. */
#define LPF_TOPK_MAX_K 1024
/* Segment s = positions [seg_ptr[s], seg_ptr[s + 1]) of score / cand (each shorter than 2^32 - 1).  Ranks a segment by
 * the 64-bit key (order-preserving uint32 of the score, -0.0 -> +0.0, NaN below -inf) << 32 | ~(position in the
 * segment), descending -- ties go to the earlier position -- and writes its first c = min(k, len) entries:
 * ids[s * k + e] = cand[.], scores[s * k + e] = score[.] (bits as stored), e >= c padded with -1 / -inf; counts[s] = c.
 * Segments of <= 256 entries: one wavefront each, a bitonic network in registers.  Longer ones: one 512-thread
 * workgroup each (a second kernel over a list the first fills); <= 4096 entries are bitonic-sorted in LDS, longer ones
 * first narrowed by an MSB-first radix select (256-bin LDS histogram per 8 bits) to <= 4096 keys.  Deterministic, no
 * float atomics.  scratch: int32[S + 1].  1 <= k <= LPF_TOPK_MAX_K. */
int lpf_segment_topk_f32(int64_t S, const int64_t *seg_ptr, const float *score, const int64_t *cand, int32_t k,
                         int32_t *scratch, int64_t *ids, float *scores, int64_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * HeaRT-style hard negatives (twohop.hip): rows of A diag(w) A, the candidate pool of a node, the rank interleave.
 * The reference only reads such negatives from files (src/util/read_datasets.py:132-146); nothing there makes them.
 * ---------------------------------------------------------------------------------------------- */
/* Sources whose expansion (sum over w in N(u) of deg(w)) exceeds this get a workgroup with dense state in the
 * workspace; the others one wavefront with the accumulators hashed in LDS.  It is also the largest threshold: a
 * larger split_threshold (or a negative one) selects it. */
#define LPF_TWOHOP_SPLIT_DEFAULT 512
/* Bytes of workspace for n_groups resident workgroups: per group and node an fp64 aa, an fp64 ra, an int32 cn and an
 * int32 stamp. */
int64_t lpf_twohop_workspace_bytes(int64_t n, int64_t n_groups);
/* Row u = sources[s] of A diag(w) A on a CSR with sorted, unique columns (values ignored): for each w in N(u) in
 * ascending order, for each c in N(w): cn[c] += 1, aa[c] += w_aa[w], ra[c] += w_ra[w]; fp64 sums in that order, rounded
 * to fp32 once; no float atomics.  The row holds the touched c in ascending id; flags bit 0 drops the members of N(u),
 * bit 1 drops u.  Sources outside [0, n) have an empty row.  The count pass writes the row lengths; the caller scans
 * them into offset (first output slot of each source, T slots in all) and the fill pass writes out_col and whichever
 * of out_cn / out_aa / out_ra is not NULL.  Both passes take the same split_threshold and flags.  scratch: int32[S + 1];
 * workspace: lpf_twohop_workspace_bytes(n, n_groups) bytes, 16-byte aligned, 1 <= n_groups <= 65535. */
int lpf_twohop_count(int64_t S, int64_t n, const int64_t *sources, const int64_t *rowptr, const int32_t *col,
                     int32_t split_threshold, int32_t flags, int32_t *scratch, void *workspace, int64_t n_groups,
                     int64_t *count, void *stream);
int lpf_twohop_fill(int64_t S, int64_t n, const int64_t *sources, const int64_t *rowptr, const int32_t *col,
                    const float *w_aa, const float *w_ra, int32_t split_threshold, int32_t flags, int32_t *scratch,
                    void *workspace, int64_t n_groups, const int64_t *offset, int64_t T, int32_t *out_col,
                    int32_t *out_cn, float *out_aa, float *out_ra, void *stream);
/* Pool of node u = nodes[i]: its two-hop row a_* (segment [a_ptr[i], a_ptr[i + 1]), built with flags = 3) united with
 * the stored entries of its row of the PPR CSR b_*, minus its row of the adjacency exc_*, minus u; ascending id.
 * lpf_pool_extra_count writes the number of PPR entries the two-hop row lacks; the caller scans them into x_ptr
 * (int64[U + 1], X = x_ptr[U]).  lpf_pool_fill writes those entries to the temporaries x_col / x_val and the pool to
 * pairs (int64 [2, T]: u, member; T = a_ptr[U] + X, the pool of node i at a_ptr[i] + x_ptr[i]) with the member's values
 * in whichever of out_cn / out_aa / out_ra / out_ppr is not NULL (cn as float; 0 where the row does not hold it). */
int lpf_pool_extra_count(int64_t U, int64_t n, const int64_t *nodes, const int64_t *a_ptr, const int32_t *a_col,
                         const int64_t *b_rowptr, const int32_t *b_col, const int64_t *exc_rowptr,
                         const int32_t *exc_col, int64_t *count, void *stream);
int lpf_pool_fill(int64_t U, int64_t n, const int64_t *nodes, const int64_t *a_ptr, const int32_t *a_col,
                  const int32_t *a_cn, const float *a_aa, const float *a_ra, const int64_t *b_rowptr,
                  const int32_t *b_col, const float *b_val, const int64_t *exc_rowptr, const int32_t *exc_col,
                  const int64_t *x_ptr, int32_t *x_col, float *x_val, int64_t X, int64_t T, int64_t *pairs,
                  float *out_cn, float *out_aa, float *out_ra, float *out_ppr, void *stream);
/* Largest list length of the rank interleave. */
#define LPF_INTERLEAVE_MAX_KH 1024
/* For node u = nodes[i]: H ranked lists ids / vals [H][U][kh] with counts [H][U] (lpf_segment_topk_f32 outputs), each
 * cut at its first value that is not > 0.  lists[i] = the first kh distinct ids of the sequence rank 1 of list 1, rank 1
 * of list 2, ..., rank 2 of list 1, ...; n_ranked[i] = how many that gave.  The rest is padding: draws d = 0, 1, 2, ...
 *   x = mix32((uint32)u * 0x9E3779B1 + (uint32)seed);  x = mix32(x ^ (uint32)(seed >> 32) ^ (d * 0x85EBCA77));  c = x % n
 *   mix32(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16      (all in uint32)
 * in order, skipping u, the members of u's row of exc_* and ids already in the list.  1 <= H <= 8,
 * 1 <= kh <= LPF_INTERLEAVE_MAX_KH.  The caller makes sure n - 1 - deg(u) >= kh (else the tail is -1 after 2^20 draws). */
int lpf_rank_interleave(int64_t U, int64_t n, const int64_t *nodes, int32_t H, int32_t kh, const int64_t *ids,
                        const float *vals, const int64_t *counts, const int64_t *exc_rowptr, const int32_t *exc_col,
                        uint64_t seed, int64_t *lists, int32_t *n_ranked, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Ranking counts (rank_metrics.hip): per positive score, the negatives that are >= it (ge) and > it (gt).  Ranks
 * (0.5 (ge + gt) + 1, src/train/evaluation.py:23-90), Hits@K, MRR, AUC and AP follow from the two.
 * Comparisons are IEEE, as in torch's (neg >= pos).sum(): a NaN negative is never counted, a NaN positive gets
 * ge = gt = 0, -0.0 == +0.0, +-inf are ordinary values.  nan_counts int64[2] (device) receives the NaNs seen among
 * the positives [0] and the negatives [1]: an overflowed selection batch scores NaN, and a metric over such scores
 * should say so.  ge / gt are written without atomics (exact, order-free); nothing is read back.
 * ---------------------------------------------------------------------------------------------- */
/* pos[P] against neg[P, K] (row stride ld_neg >= 0 floats, any base alignment): one pass over the negatives, lane
 * groups of 1 .. 64 lanes per row by K, 16-byte loads over the aligned body of every row. */
int lpf_rank_rows_f32(int64_t P, int64_t K, const float *pos, const float *neg, int64_t ld_neg, int32_t *ge,
                      int32_t *gt, int64_t *nan_counts, void *stream);
/* Bytes of workspace for sorting M negatives: the unsorted keys and rocPRIM's temporary storage, O(M); independent
 * of P (the parameter is kept so that a later layout may use it). */
int64_t lpf_rank_shared_workspace_bytes(int64_t P, int64_t M);
/* pos[P] against one shared set of M negatives, M <= 2^31 - 1.  sorted_keys uint32[M] belongs to the caller.
 * neg != NULL: the negatives (unsorted) are mapped to ordered keys (-0.0 -> +0.0, NaN -> 0xFFFFFFFF, else the sign
 * flip that makes unsigned order the IEEE order), radix-sorted into sorted_keys (workspace: 16-byte aligned,
 * workspace_bytes >= lpf_rank_shared_workspace_bytes), and the positives ranked.  neg == NULL: sorted_keys is what an
 * earlier call left there and only the positives are ranked (workspace unused) -- train, valid and test positives
 * against one set of negatives sort it once.  Two lower-bound searches per positive, the top of the tree (up to 4096
 * evenly spaced keys) in LDS. */
int lpf_rank_shared_f32(int64_t P, const float *pos, int64_t M, const float *neg, uint32_t *sorted_keys,
                        void *workspace, int64_t workspace_bytes, int32_t *ge, int32_t *gt, int64_t *nan_counts,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * Threshold profile (thresh_profile.hip): the nodes of each type every pair would select at each threshold of a grid
 * -- what thresh_cn / thresh_1hop / thresh_non1hop (src/models/link_transformer.py:241-250, 478) cost and see, for the
 * whole grid the reference searches (src/run.py:199-201) in one pass over the unfiltered graphs.
 * ---------------------------------------------------------------------------------------------- */
/* Largest number of thresholds of one call. */
#define LPF_THRESH_MAX_T 32
/* Pairs whose walked length exceeds this go to the workgroup-per-pair kernel (split_threshold < 0 selects it). */
#define LPF_THRESH_SPLIT_DEFAULT 512
/* For pair p = (a, b) = (pairs[p], pairs[pairs_ld + p]), the binary typing adjacency adj_* and the raw PPR matrix ppr_*
 * (CSRs of the same n nodes with sorted, unique columns; fp32 values, 0 where nothing is stored), candidate v has
 *   type 0 (common neighbour)  v in N(a) & N(b):                        ra = rt2(P[a,v]), rb = rt2(P[b,v])
 *   type 1 (one-hop)           v in exactly one of N(a), N(b):          ra = rt1(P[a,v]), rb = rt1(P[b,v])
 *   type 2 (>1-hop)            v in neither, P[a,v] > 0 and P[b,v] > 0: ra = rt1(P[a,v]), rb = rt1(P[b,v])
 * with the reference's fp32 round trips rt1(x) = fl(fl(x + 1) - 1), rt2(x) = fl(fl(2 x + 2) - 2) / 2, and
 *   count[p][t][j] = #{v of type t : ra >= thresholds[j] and rb >= thresholds[j]}
 * -- the nodes of type t a model with that threshold for the type selects for the pair, bit for bit.  No special case
 * for v in {a, b} or a == b.  mode_cn != 0 (mask mode "cn"): type 0 uses rt1, types 1 and 2 are empty.  A pair with an
 * id outside [0, n) counts nothing.
 * thresholds: HOST array of T values, 1 <= T <= LPF_THRESH_MAX_T, finite, >= 0, strictly ascending (else
 * LPF_ERR_INVALID, P == 0 included); they travel in the launch arguments.  Every other pointer is device memory.
 * per_pair int32[P][3][T] receives count (NULL: not written).  total int64[3][T] += sum over p of count,
 * max_per_pair int32[3][T] = max(itself, max over p), nonempty int64[3][T] += #{p : count > 0}: accumulated, so a caller
 * may chunk the pairs; it zeroes them first.
 * The pair's walks are N(a), N(b) minus N(a) and the shorter of the two PPR rows, deg(a) + deg(b) + min(|P_a|, |P_b|)
 * slots with three binary searches each: up to split_threshold slots one wavefront takes the pair, longer ones get a
 * 256-thread workgroup each (a second kernel over a list the first fills; 0 sends every non-empty pair there).
 * Counts come from ballots and integer LDS counters, the three reductions from integer atomics: the result is a pure
 * function of the input, whatever the split.  scratch: int32[P + 1].  P < 2^31 - 1. */
int lpf_threshold_profile(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *adj_rowptr,
                          const int32_t *adj_col, const int64_t *ppr_rowptr, const int32_t *ppr_col,
                          const float *ppr_val, int32_t T, const float *thresholds, int32_t mode_cn,
                          int32_t split_threshold, int32_t *scratch, int32_t *per_pair, int64_t *total,
                          int32_t *max_per_pair, int64_t *nonempty, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Batch cover (batch_cover.hip): the undirected edges a batch of train_pos ROWS removes from the typing adjacency.
 * The reference's loop drops the batch's rows and builds a symmetric adjacency from the rest
 * (src/train/train_model.py:40-45: adjmask[perm] = 0; SparseTensor.from_edge_index(train_pos[adjmask]).to_symmetric()):
 * an edge {u, v} is absent from it iff EVERY row that holds it, as (u, v) or (v, u), is in the batch.
 * ---------------------------------------------------------------------------------------------- */
/* train_pos int64[E][2]; gid int32[E] = group of row e (rows with the same {min, max} share a group), mult int32[G] =
 * rows per group; cnt int32[G] scratch, all zero on entry and all zero again when the call's work has run.
 * perm int64[B]: DISTINCT row ids, a slice of a permutation (a row named twice is counted twice and its group, seeing
 * more rows than it has, is held back).  out int64[2][B]: position i receives (min, max) of row perm[i] iff all
 * mult[g] rows of its group g are in perm, else (-1, -1) -- a group with several rows in the batch is emitted at each
 * of them; the shape is fixed and nothing is read back.
 * stats int32[4] is ADDED to, never reset: [0] positions emitted, [1] positions held back (a twin row is outside the
 * batch), [2] positions skipped -- perm[i] outside [0, E) (or a gid outside [0, G)): they write (-1, -1) and no other
 * memory is touched for them --, [3] spare.
 * Three launches in stream order (count with integer atomics, emit, reset with plain stores): emit sees the counts of
 * the whole batch.  Integers only: the result is a pure function of the input.  B, E < 2^31 - 1; B == 0 does nothing. */
int lpf_batch_cover(const int32_t *gid, const int32_t *mult, const int64_t *train_pos, int64_t E, int64_t G,
                    const int64_t *perm, int64_t B, int32_t *cnt, int64_t *out, int32_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pair distance (pair_bfs.hip): shortest-path hops between the endpoints of candidate pairs on the typing adjacency --
 * the global structural heuristic next to CN / AA / RA (the "shortest path" baseline of HeaRT / OGB comparisons).  The
 * reference has no such code.
 * ---------------------------------------------------------------------------------------------- */
/* The front kernel settles distance 2 itself when the pair's shorter row holds at most this many entries
 * (split_threshold < 0 selects it); longer rows go to the search kernel.  Chosen from the threshold sweep of
 * tools/pair_distance_time.py (profiles/pair_distance_timing.json: MI355X, collab-like graph, 32,768 pairs, 569
 * workgroups), whole-call ms at thresholds 0 / 8 / 32 / 128 / 512:
 *   held-out positives  unlimited 1.420 / 1.428 / 1.448 / 1.533 / 1.694   max_dist 3 1.113 / 1.123 / 1.144 / 1.227 / 1.386
 *   uniform random      unlimited 1.466 / 1.483 / 1.497 / 1.529 / 1.530   max_dist 3 0.916 / 0.932 / 0.944 / 0.975 / 0.975
 * Time only grows with the threshold: a lane that walks a long row alone holds its wave back, and the search
 * workgroups take a distance-2 pair in their stride.  8 stays within 2 % of the fastest entry (0) in all four columns
 * -- no more than two 5-repetition means differ by -- where 32, the value LPF_HEUR_SPLIT_DEFAULT has, costs 2-3 % and
 * 128 and above 4-19 %; unlike 0 it keeps the pairs of two short rows, a handful of probes each, off the list. */
#define LPF_BFS_SPLIT_DEFAULT 8
/* Bytes of workspace for n_groups resident workgroups: per group n 32-bit stamp words and a visit list of n + 2
 * int32: n_groups * (8 n + 8). */
int64_t lpf_pair_bfs_workspace_bytes(int64_t n, int64_t n_groups);
/* For pair p = (a, b) = (pairs[p], pairs[pairs_ld + p]) of a CSR with sorted, unique columns and a SYMMETRIC pattern
 * (values ignored; a non-symmetric pattern is outside the contract), dist[p] is, by the first rule that applies:
 *   0 when a == b (whatever the options);  -1 when an id lies outside [0, n);  the number of edges of a shortest a-b
 *   path;  -1 when there is no path.
 * flags bit 0 (ignore_direct): the stored entries (a, b) and (b, a) of this pair count as absent, nothing else changes.
 * max_dist = m > 0: a distance above m reads -1 -- exactly where(exact <= m, exact, -1) --, and the search stops as
 * soon as that is decided; max_dist <= 0: unlimited.  Stored self-loops change nothing.
 * A front kernel (one lane per pair) settles a == b, bad ids, endpoints without a usable entry, distance 1 and, for
 * pairs whose shorter row holds at most split_threshold entries, distance 2; the other pairs are listed and persistent
 * 256-thread workgroups take them by an atomic ticket, each running a bidirectional level-synchronous BFS with dense
 * epoch-stamped state over all n nodes (claims by integer compare-and-swap, appends by ballot rank).  The result is a
 * pure function of (graph, pair, options): not of the pair's position, of (a, b) versus (b, a), of split_threshold, of
 * n_groups or of timing; two runs are bitwise equal.  Integers only.
 * scratch: int32[P + 1] (the list; its counter is zeroed here).  workspace: lpf_pair_bfs_workspace_bytes(n, n_groups)
 * bytes, 16-byte aligned, 1 <= n_groups <= 65535; its stamps are zeroed here, once per call.  P < 2^31 - 1,
 * n < 2^31 - 3.  P == 0 returns LPF_OK without a launch. */
int lpf_pair_bfs(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                 const int32_t *col, int32_t max_dist, int32_t flags, int32_t split_threshold, int32_t *scratch,
                 void *workspace, int64_t n_groups, int32_t *dist, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pair walk counts (pair_walks.hip): W_l(a, b) = (A^l)[a, b] for l = 1 .. max_len <= 4 on the typing adjacency -- what
 * the Katz index sum_l beta^l W_l sums (the "Katz" baseline of HeaRT / OGB comparisons, truncated at 3 there).  The
 * reference has no such code.  Both symbols were added within ABI 16: the addition changes no existing symbol, so
 * LPF_ABI_VERSION stays.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of workspace for n_groups resident workgroups: a 16-byte header (the unit ticket), then per group one 64-bit
 * word per node (a 32-bit epoch stamp over a 32-bit payload): 16 + n_groups * 8 n. */
int64_t lpf_pair_walks_workspace_bytes(int64_t n, int64_t n_groups);
/* The CSR has sorted, unique columns and a SYMMETRIC pattern (values ignored; a non-symmetric pattern is outside the
 * contract).  W_l counts the walks of l stored entries: stored self-loops count as the entries they are, a == b is no
 * special case (W_2(a, a) = deg(a)), an id outside [0, n) gives 0 for every l.
 * The caller hands the m pairs over ORIENTED and GROUPED: pair j = (s, t) = (pairs[j], pairs[pair_stride + j]), s the
 * endpoint that is spread and t the one walked from (the counts are the same either way), and unit_ptr int32[m + 1]
 * cuts the list into units: unit u holds the pairs [unit_ptr[u], unit_ptr[u + 1]), all with the SAME s; the entries
 * after the last unit's end hold m.  Persistent 256-thread workgroups take units by an atomic ticket, spread s once
 * per unit into dense epoch-stamped state over all n nodes (the indicator of N(s) and, for max_len = 4, the two-hop
 * counts |N(s) & N(c)|, by integer atomic max and add) and walk each pair of the unit two hops from t, summing what
 * they meet in 64-bit unsigned integers.  The caller bounds the counts: W_l <= maxdeg^(l - 1) must stay below 2^63.
 * ignore_direct != 0: for a pair that is a unit of its own, every transition x -> y with {x, y} = {s, t} is skipped at
 * every step -- counting on a copy of the graph without the stored entries (s, t) and (t, s); the caller makes every
 * pair that is a stored entry a one-pair unit (a pair that is no entry is unaffected wherever it stands).
 * walks_out int64[m][max_len]: row j = W_1 .. W_max_len of pair j; pairs no unit covers are left untouched.  The result
 * is a pure function of (graph, pair, options): not of the position, the orientation, the units, n_groups or timing;
 * two runs are bitwise equal.  Integers only.
 * workspace: lpf_pair_walks_workspace_bytes(n, n_groups) bytes, 16-byte aligned; header and state are zeroed here,
 * once per call.  1 <= max_len <= 4 and 1 <= n_groups <= 65535 (checked first: LPF_ERR_INVALID whatever m is);
 * m < 2^31 - 1, n < 2^31 - 3.  m == 0 returns LPF_OK without a launch. */
int lpf_pair_walks(int64_t m, int64_t n, const int64_t *pairs, int64_t pair_stride, const int64_t *rowptr,
                   const int32_t *col, int32_t max_len, int32_t ignore_direct, const int32_t *unit_ptr,
                   void *workspace, int64_t n_groups, int64_t *walks_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pair hop counts (pair_hops.hip): how many nodes sit at distance i from one endpoint and distance j from the other --
 * what there was to select around a pair, per node class, and number for number the structure features A[d_a, d_b] and
 * B[d] that ELPH / BUDDY estimate with sketches.  The reference has no such code.  Both symbols were added within
 * ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays.
 * ---------------------------------------------------------------------------------------------- */
/* Bytes of workspace for n_groups resident workgroups: a 16-byte header (the unit ticket), then per group two 32-bit
 * words per node (one for the spread endpoint's state, one for the walk endpoint's; each a 30-bit epoch stamp over a
 * 2-bit payload): 16 + n_groups * 8 n. */
int64_t lpf_pair_hop_counts_workspace_bytes(int64_t n, int64_t n_groups);
/* The CSR has sorted, unique columns and a SYMMETRIC pattern (values ignored; a non-symmetric pattern is outside the
 * contract).  hops = k is 1 or 2.  For an endpoint u, cls_u(v) = d(u, v) if that is <= k, else k + 1 (farther than k,
 * or unreachable).  Stored self-loops change nothing; s == t is no special case (a diagonal table).
 * The caller hands the m pairs over ORIENTED and GROUPED exactly as for lpf_pair_walks: pair j = (s, t) =
 * (pairs[j], pairs[pair_stride + j]), unit_ptr int32[m + 1] cuts the list into units of one s each, the entries after
 * the last unit's end hold m.  table_out int32[m][k + 2][k + 2]: cell [i][j] of pair j =
 * |{v in [0, n) : cls_s(v) = i and cls_t(v) = j}|, the far/far cell [k + 1][k + 1] included, so a table sums to n; a
 * pair with an id outside [0, n) gets an all-zero table; pairs no unit covers are left untouched.  (t, s) gives the
 * transposed table: a caller that oriented a pair the other way round transposes it back.
 * Persistent 256-thread workgroups take units by an atomic ticket, spread s once per unit k hops into dense
 * epoch-stamped state over all n nodes (one unsigned integer atomic max per touch, which leaves a node's smallest
 * distance in any order) and expand each pair's t k hops into a second such state under a per-pair epoch; the lane
 * whose atomic max raised a word moves the node from the tally of its old class to that of its new one, which telescopes to
 * the node's final class in any order.  The far row and column follow from the class sizes (counted from the rows and
 * from the first touches of an epoch), the far/far cell from n.
 * ignore_direct != 0: for a pair that is a unit of its own, the transitions {s, t} are skipped, which is taking
 * distances on a copy of the graph without the stored entries (s, t) and (t, s); the caller makes every pair that is a
 * stored entry a one-pair unit (a pair that is no entry is unaffected wherever it stands).
 * The result is a pure function of (graph, pair, options): not of the position, the units, n_groups or timing; two runs
 * are bitwise equal.  Integers only.
 * workspace: lpf_pair_hop_counts_workspace_bytes(n, n_groups) bytes, 16-byte aligned; header and state are zeroed
 * here, once per call.  1 <= hops <= 2 and 1 <= n_groups <= 65535 (checked first: LPF_ERR_INVALID whatever m is);
 * m < 2^30 (the epoch stamps are 30 bits wide and a workgroup may take every unit and every pair), n < 2^31 - 3.
 * m == 0 returns LPF_OK without a launch. */
int lpf_pair_hop_counts(int64_t m, int64_t n, const int64_t *pairs, int64_t pair_stride, const int64_t *rowptr,
                        const int32_t *col, int32_t hops, int32_t ignore_direct, const int32_t *unit_ptr,
                        void *workspace, int64_t n_groups, int32_t *table_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Uniform negatives that avoid known edges (neg_sample.hip): K targets per source, or node pairs, drawn on the device
 * against a "known" CSR with sorted, unique int32 columns in [0, n) (values ignored; the pattern need not be
 * symmetric).  The reference draws torch.randint pairs (src/train/train_model.py:64) and has no edge-aware sampler.
 * Both symbols were added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays.
 *
 * The draw, all in uint64 (wrapping):
 *   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   G = 0x9E3779B97F4A7C15;  key(seed, i) = mix64(seed + G (i + 1));  u(seed, i, j) = mix64(key(seed, i) + G (j + 1))
 *   node(u, n) = (u * n) >> 64                      (the high half of the 128-bit product)
 * -- splitmix64 started at the slot's key.  Every output is a pure function of (seed, slot, graph, options): not of the
 * launch shape, of timing or of the other slots of the call; two runs are bitwise equal.  Integers only.
 * ---------------------------------------------------------------------------------------------- */
/* Largest K of lpf_negative_rows (the per-row hash set holds 2,048 ids) and largest max_draws of either call. */
#define LPF_NEGATIVE_MAX_K 1024
#define LPF_NEGATIVE_MAX_DRAWS (1 << 30)
#define LPF_NEGATIVE_ROW_DRAWS_DEFAULT (1 << 20)
#define LPF_NEGATIVE_PAIR_DRAWS_DEFAULT (1 << 16)
/* Row r has the source s = sources[r] and the stream c_j = node(u(seed, row_base + r, j), n), j = 0, 1, ...  A draw is
 * accepted iff c_j != s, c_j is not in row s of the CSR and c_j is no earlier accepted draw of this row.  out int64
 * [R][K], row r = the first min(K, avail) accepted draws in stream order, avail = n - deg(s) - [s not in row s]; the
 * remaining entries are -1.  A row stops after max_draws draws (1 .. LPF_NEGATIVE_MAX_DRAWS) with -1 in what is left;
 * a source outside [0, n) gives a row of -1.  short_rows (one int64, zeroed by the call, R == 0 included) counts the
 * rows with any -1.  Consequences: the K'-prefix of a row is the row for K'; a row does not depend on the other rows of
 * the call, only on its slot row_base + r -- a call over rows [lo, hi) with row_base + lo gives those rows --; a source
 * named in several rows gets a different row each time.
 * One wavefront per row, lane l of round t takes draw 64 t + l; membership is a binary search, repeats go through an LDS
 * hash set (ids claimed by compare-and-swap, the smallest draw index kept by integer atomic min: the earliest draw wins
 * within a round and against earlier ones), accepted lanes are ranked by ballot.  1 <= K <= LPF_NEGATIVE_MAX_K,
 * R < 2^31 - 1, n < 2^31 - 1 (LPF_ERR_INVALID otherwise, before anything runs). */
int lpf_negative_rows(int64_t R, int64_t n, const int64_t *sources, int32_t K, const int64_t *rowptr,
                      const int32_t *col, uint64_t seed, int64_t row_base, int32_t max_draws, int64_t *out,
                      int64_t *short_rows, void *stream);
/* Slot i draws, for j = next[i], next[i] + 1, ..., the pair a = node(u(seed, slot_base + i, 2 j), n),
 * b = node(u(seed, slot_base + i, 2 j + 1), n), accepted iff a != b and neither (a, b) nor (b, a) is a stored entry.
 * The first accepted pair goes to pairs[i], pairs[pair_stride + i] (int64) and the draw index after it to next[i]
 * (int32, input AND output: a caller makes a slot continue its stream by calling again; start it at 0; negative reads
 * as 0).  Only slots with active[i] != 0 are touched (uint8[M]; NULL: all of them).  A slot that reaches j = max_draws
 * (1 .. LPF_NEGATIVE_MAX_DRAWS) without a pair holds (-1, -1), next[i] = max_draws, and is counted in unresolved (one
 * int64, zeroed by the call, M == 0 included): a graph without a free pair ends with every slot at (-1, -1).  One lane
 * per slot.  M < 2^31 - 1, n < 2^31 - 1, pair_stride >= M. */
int lpf_negative_pairs(int64_t M, int64_t n, const int64_t *rowptr, const int32_t *col, uint64_t seed,
                       int64_t slot_base, int32_t max_draws, const uint8_t *active, int32_t *next, int64_t *pairs,
                       int64_t pair_stride, int64_t *unresolved, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Bootstrap replicates of column sums (bootstrap.hip): what confidence intervals and paired tests of the ranking
 * metrics are made of -- every metric but AP is a sum over positives of a per-positive value, so a bootstrap replicate
 * is a sum of P gathered table rows, not a re-ranking.  The reference has no such code (it repeats runs).  Both symbols
 * were added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays.
 *
 * icols int64 [P][Ci] and fcols double [P][Cf], row-major (one row is one gather); isum int64 [B][Ci], fsum double
 * [B][Cf].  For r = 0 .. B - 1 and replicate b = b0 + r:
 *   isum[r][c] = sum_{j < P} icols[idx(b, j)][c],   fsum[r][c] = sum_{j < P} fcols[idx(b, j)][c],
 *   idx(b, j) = node(u(seed, b, j), P)  -- the draw of the negatives above: slot = replicate, draw = position.
 * Replicate b is a pure function of (seed, b, tables): not of b0, B, n_groups or timing; two runs are bitwise equal.
 * Integer sums are exact (the caller keeps |icols| <= 2^32, so they cannot overflow).  An fp64 sum is added in ONE
 * order: j is cut into segments of 16,384 consecutive draws (a function of P alone); in a segment thread t of 256 adds
 * the rows of j = start + t, + 256, + 512, ... to its accumulator in that order, from +0.0; the 64 accumulators of a
 * wavefront are summed by an xor butterfly with partner distances 32, 16, 8, 4, 2, 1; the four wavefronts as
 * ((w0 + w1) + w2) + w3; the segments in ascending order, from segment 0's sum.  No float atomics.
 * Limits (LPF_ERR_INVALID otherwise, before any launch): 1 <= P < 2^31, 1 <= B < 2^31, b0 >= 0, 0 <= Ci, Cf <=
 * LPF_BOOTSTRAP_MAX_COLS, Ci + Cf >= 1, 0 <= n_groups <= 65535 (the number of workgroups; 0: eight per CU).  A table
 * whose rows are 2, 4 or 8 words and 16-byte aligned is read with 16-byte loads.
 * ---------------------------------------------------------------------------------------------- */
#define LPF_BOOTSTRAP_MAX_COLS 8
#define LPF_BOOTSTRAP_SEGMENT 16384
/* Bytes of workspace: the per-segment partial sums, B * ceil(P / LPF_BOOTSTRAP_SEGMENT) * (Ci + Cf) * 8, and 0 when P
 * is one segment (workspace may then be NULL); -1 for arguments outside the limits. */
int64_t lpf_bootstrap_workspace_bytes(int64_t P, int64_t B, int32_t Ci, int32_t Cf, int32_t n_groups);
/* workspace: 8-byte aligned, written and read by this call only.  A table with no column may be NULL. */
int lpf_bootstrap_sums(int64_t P, int64_t B, int64_t b0, uint64_t seed, const int64_t *icols, int32_t Ci,
                       const double *fcols, int32_t Cf, int64_t *isum, double *fsum, int32_t n_groups,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training step of the pair stage (pair_train.hip): the forward of get_pos_encodings
 * (link_transformer.py:182-211) and LinkAttention.message + PyG softmax + scatter-sum (layers.py:193-224) with the
 * state a backward pass needs, and the gradients torch autograd derives from them (the reference's training step,
 * src/train/train_model.py:59-77).  Entries are sorted by (type, pair); seg int64[3][bs+1] = first entry of pair p's
 * type-t segment (global entry index, seg[t][bs] = end of type t).  D in {32, 64, 128, 256}; rows 16-byte aligned.
 * Sums over entries / pairs go through per-block partials added in block order (deterministic); dZ and
 * lpf_pair_scatter_add_f32 use float atomics.  workspace: lpf_train_partial_blocks(units) * k * D floats (k below;
 * units = rows the call reduces over -- today a constant bound, 512 blocks).
 * ---------------------------------------------------------------------------------------------- */
int64_t lpf_train_partial_blocks(int64_t units);
/* H[e,:] = ReLU(LN(W1 [pa,pb] + b1)) + ReLU(LN(W1 [pb,pa] + b1)) for the entries of ONE type (w1 float[D][2],
 * b1 / gamma / beta float[D]: the first Linear and the LayerNorm of that type's ppr_encoder_* MLP). */
int lpf_pe_hidden_fwd_f32(int64_t n_entries, int32_t D, const float *w1, const float *b1, const float *gamma,
                          const float *beta, const float *pa, const float *pb, float *H, int64_t ldh, void *stream);
/* grads float[5][D] = (dW1[:,0], dW1[:,1], db1, dgamma, dbeta) from dH; workspace k = 5. */
int lpf_pe_hidden_bwd_f32(int64_t n_entries, int32_t D, const float *w1, const float *b1, const float *gamma,
                          const float *beta, const float *pa, const float *pb, const float *dH, int64_t ldh,
                          float *grads, float *workspace, void *stream);
/* out[c] = sum_r x[r, c]  (bias gradients); workspace k = 1. */
int lpf_colsum_f32(int64_t M, int32_t D, const float *x, int64_t ldx, float *out, float *workspace, void *stream);
/* k_e = Z[node_e] + KP[e]; s_e = att . leaky_relu(k_e * q[p], 0.2); out[p] = sum_e softmax_p(s)_e k_e + bias.
 * Saves the raw scores and per pair the segment max and 1 / (sum exp + 1e-16) (0 for a pair without entries). */
int lpf_pair_attention_train_fwd_f32(int64_t bs, int64_t n_entries, int32_t D, const int64_t *seg,
                                     const int32_t *e_node, const float *Z, int64_t ldz, const float *KP, int64_t ldk,
                                     const float *q, int64_t ldq, const float *att, const float *bias, float *out,
                                     int64_t ldo, float *score, float *pmax, float *pinv, void *stream);
/* Gradients of the above from dout: dK[e] (entry-major), dq[p], datt_dbias float[2][D]; workspace k = 2.  dZ: NULL (the
 * caller sums dK by node with lpf_segment_rows_sum_f32: deterministic) or float[N][lddz], zeroed by the caller, to which
 * dk_e is added at row node_e with float atomics (order of the additions not fixed). */
int lpf_pair_attention_train_bwd_f32(int64_t bs, int64_t n_entries, int32_t D, const int64_t *seg,
                                     const int32_t *e_node, const float *Z, int64_t ldz, const float *KP, int64_t ldk,
                                     const float *q, int64_t ldq, const float *att, const float *bias, const float *out,
                                     int64_t ldo, const float *score, const float *pmax, const float *pinv,
                                     const float *dout, int64_t lddo, float *dK, int64_t lddk, float *dZ, int64_t lddz,
                                     float *dq, int64_t lddq, float *datt_dbias, float *workspace, void *stream);
/* dst[key] = sum of src[order[j]] over each run of equal keys in keys_sorted (ascending j: a fixed order) -- the gradient
 * of a row gather without atomics: keys_sorted / order = the node ids of the entries sorted and the permutation that sorts
 * them, src = dK, dst = dZ (rows no key names are left untouched: zero them first).  D in {32, 64, 128, 256}. */
int lpf_segment_rows_sum_f32(int64_t n, int32_t D, const int32_t *keys_sorted, const int64_t *order, const float *src,
                             int64_t lds, float *dst, int64_t ldd, void *stream);
/* Gradient of lpf_pair_gather_f32: dX[a_k] += dsum[k] + dmul[k] * X[b_k], dX[b_k] += dsum[k] + dmul[k] * X[a_k]
 * (dmul or dsum may be NULL; dX is accumulated into). */
int lpf_pair_scatter_add_f32(int64_t bs, int32_t D, const int64_t *batch, int64_t batch_ld, int64_t n_rows,
                             const float *X, int64_t ldx, const float *dmul, int64_t ldm, const float *dsum,
                             int64_t lds, float *dX, int64_t lddx, void *stream);

/* Nearest nodes by embedding similarity (csrc/similar.hip): for each of the S query rows Q[s] the m rows v of the table
 * T [n, ldt] with the largest score(s, v) = sum_{k < D} Q[s][k] T[v][k], accumulated in fp32 on the fp32-input MFMA
 * (the order of k is the kernel's); with q_scale [S] and t_scale [n] (both or neither) the score is
 * (dot * q_scale[s]) * t_scale[v], two fp32 multiplies in that order.  No [S, n] matrix is ever held.
 * Rows: 16-byte aligned, ldq % 4 == ldt % 4 == 0, ld >= D; columns D .. ld - 1 are never used as values (NaN allowed).
 * Eligible: every v in [0, n), except -- only when src_ids [S] is given -- the members of the exclusion row of
 * src_ids[s] (exc_rowptr int64 [n + 1] / exc_col int32, rows sorted and unique; NULL: none) and, with exclude_self,
 * src_ids[s] itself.  A src_ids[s] outside [0, n) has no eligible node.
 * Ranking: the key of lpf_segment_topk_f32 with the node id in place of the position -- (ordered uint32 of the score,
 * -0.0 -> +0.0, NaN below -inf) << 32 | ~v, descending: ties go to the smaller id, NaN scores rank last.  Row s of
 * ids / scores [S, m] holds the first counts[s] = min(m, eligible) entries, best first, then -1 / -inf.  A returned
 * score is the one the key holds: -0.0 reads +0.0, a NaN the canonical quiet NaN.  The result is a pure function of
 * the inputs: it does not depend on n_ranges, on timing or on the order tiles finish in (no float atomics).
 * The grid is (source tiles) x (n_ranges node ranges, 1 .. 65535; negative: the library default, about two workgroups
 * per CU when S is small); a merge launch on the same stream joins the ranges.  workspace:
 * lpf_similar_workspace_bytes(S, m, n_ranges) bytes of device memory (a negative LPF_ERR_* for bad arguments).
 * Limits: S, n < 2^31 - 1, n >= 1, 1 <= m <= LPF_SIMILAR_MAX_M, D >= 1 (LPF_ERR_INVALID otherwise); D > 4096 returns
 * LPF_ERR_UNSUPPORTED.  Both symbols were added within ABI 16: the addition changes no existing symbol, so
 * LPF_ABI_VERSION stays. */
#define LPF_SIMILAR_MAX_M 256
int64_t lpf_similar_workspace_bytes(int64_t S, int32_t m, int32_t n_ranges);
int lpf_similar_topm_f32(int64_t S, int64_t n, int32_t D, const float *Q, int64_t ldq, const float *T, int64_t ldt,
                         const float *q_scale, const float *t_scale, const int64_t *src_ids,
                         const int64_t *exc_rowptr, const int32_t *exc_col, int32_t exclude_self, int32_t m,
                         int32_t n_ranges, void *workspace, int64_t *ids, float *scores, int64_t *counts,
                         void *stream);

/* ------------------------------------------------------------------------------------------------
 * Per-node structure (node_structure.hip): degree, core number, connected component and triangle count of every node --
 * where a pair's endpoints sit in the graph, and the numbers of a dataset table.  The reference has no such code.  The
 * five symbols were added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION stays.
 *
 * The graph is the simple undirected graph of a CSR with sorted, unique int32 columns and a SYMMETRIC pattern (values
 * ignored; a non-symmetric pattern is outside the contract): u ~ v iff u != v and v is in row u.  Stored self-loops
 * change nothing: every kernel skips col == row.  Every result is a pure function of the graph: not of the launch
 * shape, of how many launches the caller queues between read-backs, or of timing; two runs are bitwise equal.
 * Integers only; no workgroup waits on another; nothing is read back.  Common limits (LPF_ERR_INVALID otherwise,
 * before any launch): 0 <= n < 2^31 - 1, 0 <= nnz < 2^31 - 1, no NULL array (col / row may be NULL when nnz == 0).
 * n == 0 returns LPF_OK without a launch.  Row pointers outside [0, nnz] and columns outside [0, n) read as absent.
 * ---------------------------------------------------------------------------------------------- */
/* Rows longer than this are the caller's to list for lpf_core_sweep (one workgroup each); shorter ones share a
 * wavefront, eight lanes per row. */
#define LPF_CORE_LONG_ROW 64
/* hv_form of lpf_core_sweep: how a LISTED row finds H_v.  DEFAULT: an LDS histogram of min(est[u], est[v]) and a suffix
 * scan while est[v] < 4096, bisection above; BISECT: bisection on h with a workgroup count per pass, always (kept to
 * be measured against: tools/node_structure_time.py).  Both give the same estimates. */
#define LPF_CORE_FORM_DEFAULT 0
#define LPF_CORE_FORM_BISECT 1
/* degree int32[n]: the neighbours of each node other than itself. */
int lpf_node_degree(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, int32_t *degree, void *stream);
/* ONE in-place sweep of the h-index iteration on est int32[n] (the caller starts it as the degree):
 * est[v] <- min(est[v], H_v), H_v = the largest h such that at least h neighbours u have est[u] >= h.  A node whose
 * estimate drops stores it and is counted in *changed (one int32, NOT zeroed here; one integer atomic per wavefront at
 * most).  long_rows int32[n_long]: every row of more than LPF_CORE_LONG_ROW entries, each once (a row that is missing
 * is never updated).  A sweep that leaves *changed untouched has found the fixpoint, which is the core number whatever
 * mixture of old and new neighbour estimates the lanes of earlier sweeps read: estimates start as upper bounds and
 * only fall, H of upper bounds is an upper bound, and at a sweep that stored nothing every est[v] <= H_v, so {est >= k}
 * induces a subgraph of minimum degree >= k for each k. */
int lpf_core_sweep(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, const int32_t *long_rows,
                   int64_t n_long, int32_t hv_form, int32_t *est, int32_t *changed, void *stream);
/* Connected components on parent int32[n] (the caller starts it as the identity), a round = hook, then jump.
 * hook: one lane per stored entry (row[e], col[e]) -- row int32[nnz] is the row id of every entry --: where
 * parent[u] < parent[v], an agent-scope integer atomic min of parent[u] into parent[parent[v]] and into parent[v]; every
 * word that fell is counted in *changed (as above).  jump: parent[v] <- the root of v's chain (parent[x] <= x always,
 * so the chain falls strictly; at most n steps).  A hook that leaves *changed untouched ends the loop: every entry then
 * joins equal labels and every label is a root, and since labels only fall, to labels of their own component, and the
 * smallest node of a component can never be relabelled, parent[v] is the SMALLEST NODE ID of v's component. */
int lpf_components_hook(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col, int32_t *parent,
                        int32_t *changed, void *stream);
int lpf_components_jump(int64_t n, int32_t *parent, void *stream);
/* triangles int64[n]: the triangles through each node.  For every stored entry with row < col, c = |N(u) & N(v)| without
 * u and v (the sorted-row intersection of lpf_pair_heuristics_f32: the shorter row walked, the longer binary-searched)
 * is added to both endpoints with 64-bit integer atomics, and a last launch halves the sums (each triangle through a
 * node arrives over two of its edges): exact in any order.  An entry that walks more than split_threshold columns
 * (negative: LPF_HEUR_SPLIT_DEFAULT) is listed and gets a 256-thread workgroup of its own, so a hub row does not
 * serialise a wavefront.  scratch: int32[1 + nnz] (the list), written by this call only; triangles is zeroed here. */
int lpf_node_triangles(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *row, const int32_t *col,
                       int32_t split_threshold, int32_t *scratch, int64_t *triangles, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Louvain communities (community.hip; lpformer_amd/community.py): one round of local moves on a level
 * graph and the inside weight of a labelling -- the level between a node's neighbourhood and its connected component.
 * The reference has no such code.  The three symbols were added within ABI 16: the addition changes no existing symbol,
 * so LPF_ABI_VERSION stays.
 *
 * Level graph.  A CSR with sorted, unique int32 columns and a SYMMETRIC pattern, as in the section above: u ~ v iff
 * u != v and v is in row u; every kernel skips col == row.  weight int64[nnz] gives w(u, v) per stored entry (NULL: all
 * 1, level 0).  k int64[n]: k[v] = sum_{u != v} w(v, u) + s[v], s the caller's self weight (the inside weight of the
 * community a coarse node stands for; level 0: all 0).  two_m = sum_v k[v], the same at every level; two_m < 2^31, so
 * every k, tot and w_C is below 2^31 and every product below is below 2^62.  Integers only; a pure function of its
 * arguments (not of the launch shape or of timing); no workgroup waits on another; nothing is read back.  Common
 * limits (LPF_ERR_INVALID otherwise, before any launch): 0 <= n < 2^31 - 1, 0 <= nnz < 2^31 - 1, no NULL array (col /
 * row / comm of lpf_community_quality may be NULL when nnz == 0, weight always).  Row pointers outside [0, nnz] read
 * as an empty row; a column or a community outside [0, n) is skipped before it indexes.
 * ---------------------------------------------------------------------------------------------- */
/* Rows longer than this are the caller's to list for lpf_community_move (a 256-thread workgroup each); shorter ones
 * share a wavefront, eight lanes per row. */
#define LPF_COMM_LONG_ROW 64
/* Slots of the LDS table of a listed row (lds_slots): the default, and the most a workgroup's LDS holds (12 bytes per
 * slot: 48 KiB and 96 KiB of the 160 KiB). */
#define LPF_COMM_LDS_SLOTS 4096
#define LPF_COMM_LDS_SLOTS_MAX 8192
/* ONE round of local moves.  Reads the accepted state -- comm int32[n] (community ids are node ids of the level), tot
 * int64[n] (tot[c] = sum of k over the members of c), cnt int32[n] (members of c) -- and writes new_comm int32[n]:
 * the round is double-buffered.  Node v is ACTIVE iff the top bit of
 *     lpf_mix64(lpf_draw_key(seed, ((uint64_t)level << 32) + round) + G (v + 1))
 * is set (the draw of the negatives section above); an inactive node keeps comm[v].  An active node with cur = comm[v]
 * visits every community C among its neighbours' communities, w_C = sum_{u ~ v, comm[u] = C} w(v, u):
 *     gain(C) = two_m w_C - k_v (tot_C - [C == cur] k_v),      stay = gain(cur)  (w_cur = 0 with no neighbour in cur).
 * A candidate is a C != cur with gain(C) > stay, unless cnt[cur] == 1 && cnt[C] == 1 && C > cur (two singletons may
 * not swap).  The candidate of the largest gain wins, ties to the smaller id; without a candidate v stays.  *moved
 * (one int32, NOT zeroed here) counts the nodes with new_comm[v] != comm[v]: one integer atomic per wavefront at most.
 *
 * long_rows int32[n_long]: every row of more than LPF_COMM_LONG_ROW entries, each once (a row that is missing is never
 * written).  They are handled by min(n_long, 512) persistent workgroups that stride the list; a row of len entries
 * aggregates its (community, weight) pairs in an open-addressing table of T = max(64, 2^ceil(log2(2 len))) slots
 * (int32 keys claimed by compare-and-swap, int64 sums by 64-bit integer adds, at most T probes), in LDS where
 * T <= lds_slots -- a power of two in [64, LPF_COMM_LDS_SLOTS_MAX], LPF_ERR_INVALID otherwise -- and else in the
 * workgroup's region of scratch: lpf_community_workspace_bytes(n_long, longest row, lds_slots) bytes of device memory
 * (0: none needed, scratch may be NULL), ALL ZERO on entry and left all zero.  scratch_bytes is what the caller
 * passed; a row whose table neither LDS nor its region holds keeps its community.  A small lds_slots exists so that
 * tests reach the device-memory table with rows of a few hundred entries; the result is the same for every value. */
int64_t lpf_community_workspace_bytes(int64_t n_long, int64_t max_row, int32_t lds_slots);
int lpf_community_move(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, const int64_t *weight,
                       const int64_t *k, const int32_t *comm, const int64_t *tot, const int32_t *cnt, int64_t two_m,
                       uint64_t seed, int32_t level, int32_t round, const int32_t *long_rows, int64_t n_long,
                       int32_t lds_slots, void *scratch, int64_t scratch_bytes, int32_t *new_comm, int32_t *moved,
                       void *stream);
/* *inside (one int64, zeroed here) = the sum of w over the stored entries (row[e], col[e]) -- row int32[nnz] is the
 * row id of every entry -- with row != col and comm[row] == comm[col]: both directions of every inside edge.  comm may
 * hold ANY int32 labels.  Entry-parallel: at most 1,024 workgroups stride the entries, a wavefront and a workgroup
 * reduction, one 64-bit integer atomic per workgroup at most (every add lands on this one word).
 * The modularity numerator of the labelling is two_m (inside + sum_v s[v]) - sum_c tot_c^2. */
int lpf_community_quality(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col, const int64_t *weight,
                          const int32_t *comm, int64_t *inside, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Biased random walks (random_walk.hip; lpformer_amd/random_walks.py): the node2vec second-order walk by
 * rejection sampling -- what an embedding baseline (Node2Vec, DeepWalk) is trained on.  The reference has no such code,
 * and PyG's walkers live in CUDA extensions.  The symbol was added within ABI 16: the addition changes no existing
 * symbol, so LPF_ABI_VERSION stays.
 *
 * Graph.  A CSR with sorted, unique int32 columns and a SYMMETRIC pattern, as in the two sections above (values ignored;
 * a non-symmetric pattern is outside the contract).  A walk moves along stored entries; a stored self-loop is an entry
 * like any other.  Row pointers outside [0, nnz] read as an empty row; a column outside [0, n) reads as a node without
 * entries.
 *
 * Draws, those of the negatives section above with no new definition: key_w = key(seed, walk id),
 * u(j) = mix64(key_w + G (j + 1)), node(u, d) = (u * d) >> 64.
 *
 * Walk w of the call has the id walk_base + w and the start starts[w] (int64).  walk[0] = start; a start outside
 * [0, n) gives a row of -1 and a forced count of 0.  Step t = 1 .. L, with cur = walk[t - 1], d = the stored entries
 * of row cur and T = max_tries:
 *   1. d == 0: walk[t] = cur (the walk stays, as PyG pads).
 *   2. Otherwise attempt a = 0, 1, ... draws the candidate x = col[rowptr[cur] + node(u(2 ((t - 1) T + a)), d)].
 *   3. The FIRST candidate is taken without a test if t == 1, d == 1 or second_order == 0 (the caller passes 0 iff
 *      p == q == 1).
 *   4. Otherwise, with prev = walk[t - 2], x is of class RETURN (x == prev; weight 1 / p; this class wins over the
 *      next), COMMON (x is stored in row prev; weight 1) or OUT (anything else; weight 1 / q),
 *   5. and is accepted iff (u(2 ((t - 1) T + a) + 1) >> 1) < thr[class],
 *   6. thr[class] = floor(2^63 weight / max weight), computed by the caller in exact arithmetic: the heaviest class
 *      has 2^63 and always accepts.  Each threshold is at most 2^63.
 *   7. After T refused attempts the last candidate is taken and forced[w] is incremented.
 * A walk is a pure function of (seed, walk id, start, graph, L, thresholds, second_order, T): not of W, of how the
 * caller cuts its walks into calls (walk_base), of the launch shape, of form or of timing; two runs are bitwise equal.
 * Integers only; no floats on the device, no atomics; forced is per walk.
 *
 * walks int32 [L + 1][ldw] is STEP-MAJOR, walks[t * ldw + w] (a wavefront of form LANE stores one step as one
 * contiguous line), ldw >= W; forced int32 [W] or NULL.  Limits (LPF_ERR_INVALID otherwise, before any launch):
 * 0 <= n, nnz, W < 2^31 - 1, 1 <= L <= LPF_WALK_MAX_LENGTH, 1 <= max_tries <= LPF_WALK_MAX_TRIES, second_order 0 or
 * 1, a known form, no NULL array but forced (col may be NULL when nnz == 0).  W == 0 or n == 0 returns LPF_OK without
 * a launch (with n == 0 every start is outside the graph: the caller fills its -1).
 * ---------------------------------------------------------------------------------------------- */
#define LPF_WALK_MAX_LENGTH 65536
#define LPF_WALK_MAX_TRIES 65536
#define LPF_WALK_TRIES_DEFAULT 64
/* form: LANE, one lane per walk, the bounds of rows cur and prev kept in registers; GROUP8, eight lanes per walk that
 * probe row prev eight keys a round (a row of 600 entries: 3 rounds for 10).  Both give the same bits; DEFAULT is the
 * one tools/random_walks_time.py measured faster. */
#define LPF_WALK_FORM_LANE 0
#define LPF_WALK_FORM_GROUP8 1
#define LPF_WALK_FORM_DEFAULT 0
int lpf_random_walks(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, int64_t W,
                     const int64_t *starts, int64_t walk_base, int32_t L, uint64_t seed, uint64_t thr_return,
                     uint64_t thr_common, uint64_t thr_out, int32_t second_order, int32_t max_tries, int32_t form,
                     int32_t *walks, int64_t ldw, int32_t *forced, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Node2Vec's skip-gram update with negative sampling (skipgram.hip; lpformer_amd/skipgram.py): one
 * synchronous optimiser step on an embedding table, every gradient taken at the table as it stands when the step
 * begins.  The loss is PyG's Node2Vec.loss, the update torch.optim.SparseAdam; only the evaluation is new: no
 * [windows, context, dim] block, no float atomics, one fixed summation order, repeatable bits.  The reference has no
 * such code.  The three symbols were added within ABI 16: the addition changes no existing symbol, so LPF_ABI_VERSION
 * stays.
 *
 * Walk buffers.  pos and neg are STEP-MAJOR int32 [L + 1][ld], as lpf_random_walks writes them, holding Wp and Wn
 * walks; neither is unfolded in memory.  A walk has nwin = L + 2 - context windows; window (w, o) gives the pairs
 * (c, x) = (walk[o][w], walk[o + k][w]), k = 1 .. context - 1; pair id = (w nwin + o)(context - 1) + (k - 1), the
 * negative buffer's ids following the positive buffer's.  M = Mp + Mn, Mp = Wp nwin (context - 1), Mn likewise.
 * logit l = <E[c], E[x]>; with s = 1 / (1 + exp(-l)) a positive pair adds -log(s + 1e-15) / Mp to the loss and a
 * negative pair -log((1 - s) + 1e-15) / Mn.  A pair that holds an id outside [0, n) has coefficient 0 and loss 0 (it
 * still counts in Mp or Mn) and is written with both ids -1.  A pair with c == x is an ordinary pair.
 *
 * Tables are float [rows][ld] with ld >= dim, ld % 4 == 0 and a 16-byte aligned base; dim % 4 == 0,
 * 4 <= dim <= LPF_SKIPGRAM_MAX_DIM.  Every entry returns LPF_ERR_INVALID before any launch for arguments outside its
 * limits, and LPF_OK without a launch for an empty call.  No id read from a buffer indexes anything before it is
 * range-checked.
 * ---------------------------------------------------------------------------------------------- */
#define LPF_SKIPGRAM_MAX_DIM 512
/* occurrences per chunk of lpf_skipgram_grad_rows_f32: part of its result's definition */
#define LPF_SKIPGRAM_CHUNK 128
/* windows per workgroup of lpf_skipgram_coef_f32: partial holds ceil((Wp + Wn) nwin / this) sums */
#define LPF_SKIPGRAM_BLOCK_WINDOWS 16
/* coef float [M]: g = dloss/dl per pair, 1 / Mp or 1 / Mn folded in -- the logit in fp32 (one order per dim), the
 * sigmoid and the quotient in fp64 from it, rounded once.  centre, other int32 [M]: the pair's ids (-1, -1 and g = 0
 * for a bad pair).  partial double [partial_len >= ceil((Wp + Wn) nwin / LPF_SKIPGRAM_BLOCK_WINDOWS)]: the
 * workgroups' loss sums; *loss (one double) is their sum in one fixed order.  A group of 16 lanes per window loads the
 * centre row once and walks its context - 1 partners; rows are read as 16-byte loads.
 * Limits: 0 <= n < 2^31 - 1, 1 <= L <= LPF_WALK_MAX_LENGTH, 2 <= context <= L + 1, 0 <= Wp <= ldp, 0 <= Wn <= ldn,
 * M < 2^31 - 1.  Wp + Wn == 0: LPF_OK, nothing written (*loss included). */
int lpf_skipgram_coef_f32(int64_t n, int32_t dim, const float *table, int64_t ldt, int32_t L, int32_t context,
                          const int32_t *pos, int64_t Wp, int64_t ldp, const int32_t *neg, int64_t Wn, int64_t ldn,
                          float *coef, int32_t *centre, int32_t *other, double *partial, int64_t partial_len,
                          double *loss, void *stream);
/* grad float [U][ldg]: grad[u] = sum over the occurrences e in [seg[u], seg[u + 1]) of coef[occ_pair[e]] *
 * E[occ_other[e]], one fused multiply-add per element and occurrence, IN THE LISTED ORDER within a chunk: the segment
 * is cut at seg[u] + j LPF_SKIPGRAM_CHUNK, each chunk is summed from zero by one wavefront, and the chunks' rows are
 * added in chunk order.  The result is a function of the inputs and of that constant only -- not of groups (the
 * number of workgroups; 0: one wavefront per LPF_SKIPGRAM_CHUNK occurrences of the list), of the launch shape or of
 * timing.  The caller lists, for pair i, the occurrences (row c_i, other x_i, pair i) and (row x_i, other c_i,
 * pair i), sorted by row and within a row by occurrence id; seg int64 [U + 1] ascending from 0 to n_occ.  An
 * occurrence whose other is outside [0, n) or whose pair is outside [0, M) adds nothing; segment offsets are clamped
 * to [0, n_occ].  scratch float [scratch_rows >= ceil(n_occ / LPF_SKIPGRAM_CHUNK)][ldg], 16-byte aligned: the later
 * chunks' rows.  Reads the table, writes grad and scratch only.  U == 0: LPF_OK without a launch. */
int lpf_skipgram_grad_rows_f32(int64_t n, int32_t dim, const float *table, int64_t ldt, int64_t M, const float *coef,
                               int64_t n_occ, const int32_t *occ_other, const int32_t *occ_pair, int64_t U,
                               const int64_t *seg, float *grad, int64_t ldg, float *scratch, int64_t scratch_rows,
                               int32_t groups, void *stream);
/* torch.optim.SparseAdam on the U DISTINCT rows rows[u] of table, exp_avg and exp_avg_sq ([n][ldt], [n][lds],
 * [n][lds]), in place, from grad [U][ldg]:  m += (g - m)(1 - beta1);  v += (g g - v)(1 - beta2);
 * param -= lr sqrt(bias2) / bias1 * m / (sqrt(v) + eps).  step >= 1 is the global step count of this update, and the
 * caller passes bias1 = 1 - beta1^step and bias2 = 1 - beta2^step computed in double (both in (0, 1]).  A listed row
 * outside [0, n) is skipped; rows not listed are untouched.  0 <= beta < 1, lr, eps >= 0; 1 - beta1, 1 - beta2, eps
 * and the step size are rounded to fp32 once, the arithmetic is fp32.  U == 0 or n == 0: LPF_OK without a launch. */
int lpf_sparse_adam_rows_f32(int64_t n, int32_t dim, float *table, int64_t ldt, float *exp_avg, float *exp_avg_sq,
                             int64_t lds, int64_t U, const int32_t *rows, const float *grad, int64_t ldg, double lr,
                             double beta1, double beta2, double eps, int64_t step, double bias1, double bias2,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Common-neighbour pooling (cn_pool.hip; lpformer_amd/ncn.py): the sum of a table's rows over the common
 * neighbours of a pair -- what NCN (Wang, Yang, Zhang: Neural Common Neighbor with Completion for Link Prediction)
 * scores a pair from, and LPFormer's pairwise stage with uniform attention on the common neighbours only.  The
 * reference counts common neighbours with dense adj[edge].to_dense() rows ([BS, N] per batch, src/train/eval.py:21-41)
 * and has no such pooling.  Both symbols were added within ABI 16: the addition changes no existing symbol, so
 * LPF_ABI_VERSION stays.
 *
 * Graph: the CSR lpf_pair_heuristics_f32 reads -- sorted, unique int32 columns, a binary pattern.  For pair
 * p = (a, b) = (pairs[p], pairs[pairs_ld + p]):  C(p) = N(a) & N(b) in ascending node id, u_1 < ... < u_k.  A pair with
 * an id outside [0, n) has k = 0; a == b gives C = N(a) (what lpf_pair_heuristics_f32 counts); a node is in its own
 * neighbourhood only where the graph stores a self-loop, so a positive pair's own edge never enters its pool.
 *   pool[p] = sum_j ( sum_{i in chunk j} w[u_i] T[u_i] ),  chunk j = the entries [j C, (j + 1) C) of C(p),
 * C = LPF_CN_POOL_CHUNK: each chunk is summed from zero in ascending order, one fp32 fused multiply-add per element
 * and entry, and the chunks' rows are added in chunk order to a total that starts at zero.  The result is a function
 * of ({a, b}, graph, T, w) and of that constant only -- not of the pair's position, of (a, b) versus (b, a), of
 * split_threshold, of the launch shape or of timing; no float atomics.  The pair walks its shorter row and
 * binary-searches the other; walked rows of at most split_threshold entries (negative: LPF_HEUR_SPLIT_DEFAULT) are
 * flattened 64 probes per wavefront, longer ones get a 256-thread workgroup each, and the two classes agree bitwise.
 *
 * Tables are float [rows][ld] with ld >= dim, ld % 4 == 0 and a 16-byte aligned base; dim % 4 == 0,
 * 4 <= dim <= LPF_CN_POOL_MAX_DIM.  0 < P < 2^31 - 1, 0 < n <= INT32_MAX.  Every entry returns LPF_ERR_INVALID before
 * any launch for arguments outside its limits, and LPF_OK without a launch for P == 0.  No id read from memory indexes
 * anything before it is range-checked: a common column outside [0, n) (a malformed graph) counts in cn, is listed by
 * lpf_cn_entries as it stands and takes its place in its chunk, but adds nothing to the pool.
 * ---------------------------------------------------------------------------------------------- */
#define LPF_CN_POOL_MAX_DIM 512
/* common neighbours per chunk of lpf_cn_pool_f32: part of its result's definition */
#define LPF_CN_POOL_CHUNK 64
/* pool float [P][ldp]: every row is written, zeros where k = 0; what lies behind dim in a row is left alone.  w float
 * [n] or NULL (1.0).  table float [n][ldt].  cn int32 [P] or NULL: k.  scratch int32 [P + 1] (the long-pair list).
 * The intersection and the row gather are one pass: no list of entries exists in memory. */
int lpf_cn_pool_f32(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                    const int32_t *col, const float *w, int32_t dim, const float *table, int64_t ldt,
                    int32_t split_threshold, int32_t *scratch, float *pool, int64_t ldp, int32_t *cn, void *stream);
/* C(p) itself: node[seg[p] + i] = u_(i + 1).  seg int64 [P + 1]: the exclusive scan of cn (the caller's), n_ent the
 * length of node, 0 <= n_ent < 2^31 - 1.  Pair p writes its first seg[p + 1] - seg[p] entries and nothing else: the
 * segment offsets are clamped to [0, n_ent] (and seg[p + 1] to seg[p] from below), as lpf_skipgram_grad_rows_f32
 * clamps its own, so a seg that disagrees with the graph writes inside its own segments only and never outside
 * node[0 .. n_ent); where a segment is longer than C(p), its tail is left as it was.  n_ent == 0: LPF_OK without a
 * launch.  scratch int32 [P + 1]. */
int lpf_cn_entries(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                   const int32_t *col, int32_t split_threshold, int32_t *scratch, const int64_t *seg, int64_t n_ent,
                   int32_t *node, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Host side (liblpformer_host.so)
 * ---------------------------------------------------------------------------------------------- */

/* Approximate personalised PageRank for every source node: calc_ppr (src/util/calc_ppr_scores.py:136-192)
 * followed by create_sparse_ppr_matrix (:221-241).  Same LIFO push order and float64 arithmetic per source, so
 * the produced index sets and fp32 values are bit-identical; OpenMP over sources (num_threads <= 0: all cores).
 * indptr/indices: CSR of the coalesced directed edge list (get_ppr_matrix, :111-117), host memory.
 * out_rowptr: caller-provided int64[n+1].  *out_col / *out_val: malloc'ed by the library, sized out_rowptr[n],
 * rows sorted by column; release both with lpf_host_free. */
int lpf_ppr_push_cpu(int64_t n, const int64_t *indptr_host, const int32_t *indices_host, double alpha, double eps,
                     int64_t *out_rowptr_host, int32_t **out_col_host, float **out_val_host, int32_t num_threads);

/* The same push for the sources `sources_host[0 .. n_src)` only (ids in [0, n), strictly ascending): out_rowptr is
 * int64[n_src + 1] and row k of the result belongs to the k-th source.  Host twin of lpf_ppr_push_f64_sources. */
int lpf_ppr_push_cpu_sources(int64_t n, const int64_t *indptr_host, const int32_t *indices_host, double alpha,
                             double eps, int64_t n_src, const int32_t *sources_host, int64_t *out_rowptr_host,
                             int32_t **out_col_host, float **out_val_host, int32_t num_threads);

void lpf_host_free(void *p);
int lpf_host_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LPFORMER_HIP_H */
