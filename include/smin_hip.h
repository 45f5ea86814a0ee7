/* smin_hip.h -- C ABI of the MI355X (gfx950) SMIN hot path: cross-modal fusion + 2D temporal
 * proposal scoring of ChanukyaVardhan/Video-Moment-Localization (reference models.py).
 *
 * The reference has no FFI of its own (pure PyTorch): its de-facto operator boundary is
 * the nn.Module surface of models.py.  Each entry point below replaces the body of one of those
 * modules' forward() (cited per function) for fwd and for the autograd backward torch would derive.
 * The Python host (video-moment-localization_amd/) binds these with ctypes and keeps the reference's
 * module/ctor/forward/state_dict surface.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated; `stream` is a hipStream_t.
 *   - all calls are asynchronous on `stream`, allocate nothing and never synchronise (graph-capturable);
 *     scratch comes from the caller-provided workspace `ws`; each entry point that takes one names the query for its size
 *     (smin_<entry>_ws_bytes or _workspace_bytes: a pure host function of the entry point's own shape arguments).
 *   - return 0 on success, a positive hipError_t, or a negative code for a rejected argument.
 *   - requirements: D % 4 == 0, dl % 16 == 0, 16 <= dl <= 128, 2 <= C <= 4, Nq <= 32.
 *
 * Packed valid-cell layout: the L x L map is stored as a list of N cells sorted by
 * (b, i, j):  cells[n] = {b, i, j, m} (int32 x4, m = moment_mask[b,i,j]);
 *             row_ptr[b*L+i] .. row_ptr[b*L+i+1] = the cells of start-snippet row (b, i)  (B*L+1 ints);
 *             cellmap[b][i][j] = n or -1.
 * Per-cell tensors: f_c [N][C][D], f_m [N][D].  With moment-mask driven lists (m == 1 everywhere) this
 * is bit-equivalent to the reference's dense (B,L,L,..) tensors, whose masked cells are exactly zero;
 * with a list of all B*L*L cells it reproduces the dense sub-module seams for arbitrary inputs.
 */
#ifndef SMIN_HIP_H
#define SMIN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): smin_build_cells_n, smin_step_prologue, smin_lstm_pack_layers, smin_bilstm_layer_bwd_weights, smin_video_encoder_gate
 * (smin_video_encoder_fwd with fs == f == NULL), smin_lstm_cluster_error; new trailing arguments of smin_gate_bwd (cells, boundary
 * A, boundary dout), smin_moment_unit_bwd[_x1h] (dfb_acc) and smin_build_targets; smin_score_map_bwd may be issued as two halves;
 * content attention requires dl % 16 == 0; round-2 changes that were not versioned: smin_linear_rows_bwd accepts dW == NULL,
 * smin_video_encoder_bwd / smin_bilstm_layer_bwd may be issued as two halves */
/* additions within 2 (new entry points only; no existing signature or behaviour changed, so a caller built against 2 is unaffected
 * and the number stays): gradients of the model's inputs -- smin_video_encoder_bwd_input (dx of the video features from the inputs
 * half's workspace), smin_sample_clips_bwd, smin_embed_tokens_bwd and smin_embed_tokens_bwd_workspace_bytes (deterministic backward
 * passes of the device feeding path); long-video retrieval over overlapping windows -- smin_sample_windows (clip resampling of
 * arbitrary, possibly overlapping row ranges), smin_merge_window_moments (greedy NMS of per-window top-k moments in absolute
 * time), and a masks-only use of smin_build_targets (sm == NULL); forward-only scoring -- smin_score_tail_fwd and
 * smin_score_tail_ws_bytes (the last layer's moment unit and the map's score head as row dots); an epoch's metric and loss totals
 * kept on the device -- smin_epoch_meter_update and smin_epoch_meter_ws_bytes; the metric of merged spans against ground-truth
 * spans -- smin_span_ious, smin_span_meter_update and smin_span_meter_ws_bytes; the optimizer update -- smin_adam_step, smin_grad_norm
 * and smin_adam_ws_bytes; row-sparse training of the word table -- smin_embed_tokens_bwd_rows, smin_embed_tokens_bwd_rows_workspace_bytes
 * (the table gradient as its distinct rows) and smin_row_adam_step (a lazy Adam step over those rows); the merge of several such row
 * lists into one -- smin_row_lists_merge and smin_row_lists_merge_workspace_bytes (data-parallel ranks, micro-batches); with it
 * smin_row_adam_step takes lists of up to 65536 slots where it took 4096 (it rejected longer ones before any launch); corpus search
 * over banks of encoded videos and queries -- smin_pair_assemble (the backbone's outputs of indexed pairs) and smin_corpus_topk (one
 * ranked list per query across videos); evaluation of corpus search -- smin_search_merge (ranked lists of disjoint video shards into
 * one list per query) and smin_corpus_meter_update with smin_corpus_meter_ws_bytes (VCMR and VR recall into the epoch meter's kind of
 * accumulator); training through shared banks -- smin_pair_assemble_bwd and smin_pair_assemble_bwd_workspace_bytes (the adjoint of
 * smin_pair_assemble: the pairs' gradients summed onto their videos and queries in a fixed order); hard-negative mining on the device
 * -- smin_mine_pairs and smin_mine_pairs_ws_bytes (each query's own video and its highest-scoring wrong ones as the pair lists and both
 * groupings smin_pair_assemble_bwd reads); a contrastive loss over a pair plan -- smin_pair_rank_fwd, smin_pair_rank_bwd and
 * smin_pair_rank_ws_bytes (each query's own video ranked above the wrong ones it was paired with); corpus search over
 * banks of windows of long videos -- smin_corpus_span_topk (one ranked list of span-valued moments per query across videos); an exact
 * workspace size query for each entry point that had none -- smin_proposal_map_fwd_ws_bytes, smin_proposal_map_bwd_ws_bytes,
 * smin_clip_window_means_fwd_ws_bytes, smin_clip_window_means_bwd_ws_bytes, smin_gate_bwd_ws_bytes, smin_moment_unit_bwd_ws_bytes,
 * smin_score_map_bwd_ws_bytes and smin_content_unit_bwd_ws_bytes (smin_workspace_bytes is now their maximum); merging the span lists
 * of sharded window banks -- smin_span_search_merge (smin_search_merge for smin_corpus_span_topk's lists, as a one-pass rank); video ranking
 * by the pooled pair score -- smin_pair_pool, smin_group_pool, smin_video_rank and smin_moment_reweight (the score the contrastive loss
 * trains, read at inference: a video ranking, a weight on each video's moments and a cut to the best videos); that weight and cut
 * across shards -- smin_search_merge_weighted and smin_span_search_merge_weighted (shard lists that carry their unweighted scores,
 * merged under the video weights and ranks of all the shards' videos); a listwise soft-target loss over a pair plan --
 * smin_pair_distill_fwd and smin_pair_distill_ws_bytes (a query's softmax over its pair scores pulled towards a teacher's, through
 * smin_pair_rank_bwd); the window plan of a pruned window search -- smin_window_expand (each query's surviving videos expanded to the
 * (query, window) list and its group pointers on the device) */
#define SMIN_HIP_ABI_VERSION 2

int smin_abi_version(void);
/* Arithmetic of the dense contractions (forward maps, input gradients, weight gradients):
 *   0 (default) exact fp32 on v_mfma_f32_32x32x2_f32;
 *   1 split-bf16: operands split into hi+lo bf16 on the fly, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with
 *     fp32 accumulation (~2^-16 relative per product, ~1e-5 on a dot product);
 *   2 plain bf16: operands rounded to bf16 once, fp32 accumulation (~4e-3 relative per product; BASELINE.json configs[1]);
 *   3 fp32 emulated on the bf16 matrix cores: operands split EXACTLY into three bf16 pieces (3 x 8 mantissa bits), six
 *     products (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid) accumulated in fp32, smallest first; the three dropped terms
 *     are <= 2^-26 relative per product, below fp32's own product rounding -- results agree with mode 0 to fp32 rounding.
 * Process-wide; returns 0 or -1 for an unknown mode. */
int smin_set_gemm_mode(int mode);
int smin_get_gemm_mode(void);
/* Launch timing for benchmarks: while enabled, chosen launches inside the entry points below are bracketed by HIP events
 * recorded on the stream the launch goes to (tags: SMIN_PROF_*).  smin_prof_enable(1) clears earlier records;
 * smin_prof_read waits for the recorded events, writes up to `cap` (tag, milliseconds) pairs in launch order and returns
 * how many it wrote (or a negative code).  Off by default; costs two event records per tagged launch when on. */
#define SMIN_PROF_MOMENT_FWD 1   /* moment unit, forward contraction   mu = [x1 | mean_c f_c] Wcat^T          */
#define SMIN_PROF_MOMENT_DX 2    /* moment unit, input gradient        dX = dmu Wcat                            */
#define SMIN_PROF_MOMENT_DW 3    /* moment unit, weight gradient       dWcat = dmu^T [x1 | mean_c f_c]         */
#define SMIN_PROF_ATTN_FWD 4     /* content attention core, forward                                             */
#define SMIN_PROF_ATTN_BWD 5     /* content attention core, backward (all its launches)                         */
int smin_prof_enable(int on);
int smin_prof_read(int32_t* tags, float* ms, int cap);
/* "gfx950" -- the only code object in the library */
const char* smin_target_arch(void);
/* The old catch-all scratch size, kept for callers built against it; new code asks the entry point's own query.  It is the largest
 * of smin_content_unit_bwd_ws_bytes(N, B, C, D, dl, 0), smin_moment_unit_bwd_ws_bytes(N, B, L, D) and smin_score_map_bwd_ws_bytes(N, B,
 * L, D); a query that rejects the arguments contributes nothing.  It was never given the map side and takes L = 64: that matters to the
 * score map's term alone, and a list of N >= B * L cells is covered at any L by the moment unit's term.  (Nq is not used.) */
size_t smin_workspace_bytes(int N, int B, int C, int D, int dl, int Nq);

/* ---- ProposalGeneration.forward (models.py:115-126) with compute_content_matrix (models.py:88-98)
 * as index arithmetic: fc[n,c,:] = mean of f[b, start..start+cs) per clip, fm = mean_c fc (divides by C),
 * fb = AvgPool1d(T/L) over time.  f [B][T][D]; fc [N][C][D]; fm [N][D]; fb [B][L][D].
 * ws_bytes >= smin_proposal_map_fwd_ws_bytes(B, T, D) (0 = arguments rejected: D % 4, D > 2048). */
size_t smin_proposal_map_fwd_ws_bytes(int B, int T, int D);
int smin_proposal_map_fwd(void* stream, const float* f, const int32_t* cells, int N, int B, int T, int L, int C, int D,
                          float* fc, float* fm, float* fb, void* ws, size_t ws_bytes);
/* (any of fc/fm/fb may be NULL = not wanted) */
/* The clip-boundary table of a geometry (T, L, C): which clip of which (i, j) starts / ends at each frame -- the
 * sparsity pattern of the reference's cached content matrix (models.py:88-98, 110).  Build once per geometry: call
 * with table == NULL to get counts [T]; form the exclusive prefix offsets [T+1]; call with counts == NULL to fill
 * table (8 bytes per entry, offsets[T] entries). */
int smin_clip_event_table(void* stream, int T, int L, int C, int32_t* counts, const int32_t* offsets, void* table);
/* df [B][T][D] = d/df of the three outputs (any of dfc/dfm/dfb may be NULL = zero).
 * ws_bytes >= smin_proposal_map_bwd_ws_bytes(B, T, D) (0 = arguments rejected: D % 4, D > 2048); the workspace is neither read nor
 * checked when N == 0 or dfc == dfm == NULL.
 * ev_offsets / ev_table: the geometry's clip-boundary table (NULL, NULL = derive the boundaries in-kernel, slower). */
size_t smin_proposal_map_bwd_ws_bytes(int B, int T, int D);
int smin_proposal_map_bwd(void* stream, const float* dfc, const float* dfm, const float* dfb,
                          const int32_t* cells, const int32_t* row_ptr, const int32_t* cellmap,
                          int N, int B, int T, int L, int C, int D, float* df, void* ws, size_t ws_bytes,
                          const int32_t* ev_offsets, const void* ev_table);

/* ---- Gated moment feature shared by ContentUnit (models.py:272-274) and BoundaryUnit (models.py:191):
 *   hbar[n,:] = sigmoid(f_m[n,:] * f_s[b,:]) * f_m[n,:]          hbar [N][D]
 * backward: dfm [N][D], dfs [B][D].  hbar and f_m usually have several consumers (content unit, boundary unit, the
 * content stream's running sum; f_m also passes through to the moment unit's residual): dhbar / dres are HOST arrays of
 * n_dhbar (1..4) / n_dres (0..4) device pointers [N][D] whose sum is the gradient of hbar / is added to dfm. */
int smin_gate_fwd(void* stream, const float* fm, const float* fs, const int32_t* cells, int N, int D, float* hbar);
/* the same, and hsum_out = hsum_in + hbar [N][D] (running sum over layers, read by the next layers' gate term of chat) */
int smin_gate_fwd_sum(void* stream, const float* fm, const float* fs, const int32_t* cells, int N, int D, float* hbar, const float* hsum_in,
                      float* hsum_out);
/* boundary_A [B][L][L], boundary_dout [B][L][D] (both or neither; cells [N][4] then required): the boundary unit's consumer of hbar,
 * f_bm[b,i] = sum_j A[b,i,j] hbar[b,i,j] (models.py:191-194), enters as A[b,i,j] * boundary_dout[b,i,:] formed on the fly -- pass the
 * unit's saved attention A and the gradient of its output, and call smin_boundary_unit_bwd with dhbar == NULL.
 * ws_bytes >= smin_gate_bwd_ws_bytes(B, L, D) (0 = arguments rejected: D % 4). */
size_t smin_gate_bwd_ws_bytes(int B, int L, int D);
int smin_gate_bwd(void* stream, const float* const* dhbar, int n_dhbar, const float* const* dres, int n_dres,
                  const float* fm, const float* fs, const int32_t* row_ptr,
                  int N, int B, int L, int D, float* dfm, float* dfs, void* ws, size_t ws_bytes,
                  const int32_t* cells, const float* boundary_A, const float* boundary_dout);

/* ---- ContentUnit.forward (models.py:242-276) incl. ContentAttention.forward (models.py:207-226).
 * Query-side per-sample operands are prepared by the host (O(B*Nq*dl) work):
 *   what [B][Nq][dl] = linear_w_hat(f_w) * query_mask          shat [B][dl] = linear_s_hat(f_s)
 *   Mq   [B][Nq][dl] = W_k(what) @ W_q.weight                   uq   [B][Nq] = W_k(what) @ W_q.bias
 *   (so that  W_q(c_hat) . W_k(what)^T  ==  c_hat . Mq^T + uq  -- the per-cell dl x dl projection folds away)
 *   qmask [B][Nq] fp32 0/1;  hbar from smin_gate_fwd.
 * Outputs: fc_out [N][C][D], fcmean [N][D] = mean_c fc_out (consumed by the moment unit);
 * saved for backward: chat [N*C][dl], cchat [N*C][dl].
 * last != 0 (final SMI layer: nothing consumes fc_out itself, models.py:372-375): fc_out is not written (may be
 * NULL), cchat receives mean_c cchat [N][dl] and linear_c runs on N rows; fcmean_in [N][D] = mean_c fc (the
 * previous layer's fcmean, or the proposal map's f_m) is required. */
int smin_content_unit_fwd(void* stream, const float* fc, const float* hbar, const int32_t* cells, const int32_t* row_ptr,
                          int N, int B, int L, int C, int D, int dl, int Nq,
                          const float* Wch, const float* bch, const float* Mq, const float* uq,
                          const float* what, const float* shat, const float* qmask, const float* Wc, const float* bc,
                          const float* fcmean_in, int last,
                          float* fc_out, float* fcmean, float* chat, float* cchat);
/* Backward.  dfc_out may be NULL (last layer: only the moment unit consumes fc_out, through fcmean); pass the
 * same `last` as in forward (then dfc_out must be NULL and cchat is the [N][dl] clip mean).
 * WcT [dl][D] and WchT [D][dl] are transposed copies of the weights.
 * Gradients: dfc [N][C][D], dhbar [N][D], dWch [dl][D], dbch [dl], dMq [B][Nq][dl], duq [B][Nq],
 * dwhat [B][Nq][dl], dshat [B][dl], dWc [D][dl], dbc [D].
 * ws_bytes >= smin_content_unit_bwd_ws_bytes(N, B, C, D, dl, last) (0 = arguments rejected: D % 4, dl % 16, dl outside 16..128,
 * C outside 2..4); N == 0 is a no-op that reads no workspace. */
size_t smin_content_unit_bwd_ws_bytes(int N, int B, int C, int D, int dl, int last);
int smin_content_unit_bwd(void* stream, const float* dfc_out, const float* dfcmean,
                          const float* fc, const int32_t* cells, const int32_t* row_ptr,
                          int N, int B, int L, int C, int D, int dl, int Nq,
                          const float* WchT, const float* Mq, const float* uq,
                          const float* what, const float* shat, const float* qmask, const float* WcT,
                          const float* chat, const float* cchat,
                          float* dfc, float* dhbar, float* dWch, float* dbch, float* dMq, float* duq,
                          float* dwhat, float* dshat, float* dWc, float* dbc, void* ws, size_t ws_bytes, int last);

/* ---- BoundaryUnit.forward, the map-sized part (models.py:190-194):
 *   fbm[b,i,:] = sum_j A_b[b,i,j] * hbar[(b,i,j),:]
 * A_b [B][L][L] comes from the L x L boundary self-attention (models.py:164-188), which the host runs
 * as plain library GEMMs.  fbm [B][L][D]. */
int smin_boundary_reduce_fwd(void* stream, const float* Ab, const float* hbar, const int32_t* cells,
                             const int32_t* row_ptr, int N, int B, int L, int D, float* fbm);
/* dAb [B][L][L] (zero where no cell), dhbar [N][D]. */
int smin_boundary_reduce_bwd(void* stream, const float* dfbm, const float* Ab, const float* hbar,
                             const int32_t* cells, const int32_t* row_ptr, int N, int B, int L, int D,
                             float* dAb, float* dhbar);

/* ---- BoundaryUnit.forward, whole unit (models.py:164-196) with its word attention Attention.forward (models.py:137-154):
 *   out = (A_b f_b) * lm + f_b + sum_j A_b[i,j] hbar[(i,j)],  A_b = softmax(mask(bq bq^T / sqrt(D))) * lm,
 *   bq = f_b * (softmax(mask(W_q f_b . (W_k f_w)^T / sqrt(D))) f_w * lm + f_s).
 * fb [B][L][D], fw [B][Nq][D], fs [B][D], qmask [B][Nq], lmask [B][L] fp32 0/1; Wq, Wk [D][D] (+ biases).
 * Saved for backward (caller-allocated): Qb, baq, bqv [B][L][D], Kb [B][Nq][D], P [B][L][Nq], A [B][L][L].
 * P is also the boundary unit's Attention.attn_weights (models.py:137-154), every row i (length_mask 0 included). */
int smin_boundary_unit_fwd(void* stream, const float* fb, const float* fw, const float* fs, const float* hbar,
                           const int32_t* cells, const int32_t* row_ptr, int N, int B, int L, int Nq, int D,
                           const float* Wq, const float* bq, const float* Wk, const float* bk,
                           const float* qmask, const float* lmask,
                           float* out, float* Qb, float* Kb, float* P, float* baq, float* bqv, float* A);
/* WqT, WkT: transposed weights.  Gradients: dfb, dfw, dfs, dhbar [N][D], dWq, dbq, dWk, dbk.
 * ws_bytes >= smin_boundary_unit_bwd_ws_bytes(B, L, Nq, D).  Forward and backward take 1 <= L <= 8192. */
size_t smin_boundary_unit_bwd_ws_bytes(int B, int L, int Nq, int D);   /* 0 = arguments rejected */
int smin_boundary_unit_bwd(void* stream, const float* dout, const float* fb, const float* fw, const float* fs, const float* hbar,
                           const int32_t* cells, const int32_t* row_ptr, int N, int B, int L, int Nq, int D,
                           const float* WqT, const float* WkT, const float* qmask, const float* lmask,
                           const float* Qb, const float* Kb, const float* P, const float* baq, const float* bqv, const float* A,
                           float* dfb, float* dfw, float* dfs, float* dhbar, float* dWq, float* dbq, float* dWk, float* dbk,
                           void* ws, size_t ws_bytes);

/* ---- MomentUnit.forward (models.py:288-303): two 1x1 convs fused into one K = 2D contraction
 *   mu[n,:] = m * ( [fb[b,i]*fb[b,j] | fcmean[n]] @ Wcat^T + bcat ) + fm[n,:]
 * Wcat [D][2D] = [conv_layer_fb.weight | conv_layer_fc.weight], bcat [D] = sum of the two biases. */
int smin_moment_unit_fwd(void* stream, const float* fcmean, const float* fm, const float* fb, const int32_t* cells,
                         int N, int B, int L, int D, const float* Wcat, const float* bcat, float* mu,
                         const float* x1 /* nullable [N][D] = f_b[i]*f_b[j] from smin_pair_product: the contraction then
                                            reads two plain matrices (pass it to smin_moment_unit_bwd as well) */);
/* x1[n][:] = f_b[b][i][:] * f_b[b][j][:]  -- the pair half of the moment unit's left operand (models.py:292-294) */
int smin_pair_product(void* stream, const float* fb, const int32_t* cells, int N, int L, int D, float* x1);
/* WcatT [2D][D].  dfcmean [N][D], dfb [B][L][D], dWcat [D][2D], dbcat [D]; the residual gradient
 * d mu / d fm is the identity and is left to the caller (dfm += dmu).  Either half may be skipped: dfcmean == dfb == NULL
 * computes only the weight gradients, dWcat == dbcat == NULL only the input gradients (the halves share nothing but
 * dmu, so a host may run them on two streams; each call needs its own workspace).
 * ws_bytes >= smin_moment_unit_bwd_ws_bytes(N, B, L, D) (0 = arguments rejected: D % 4, D > 2048): one layout for either half, for
 * the whole, and for smin_moment_unit_bwd_x1h. */
size_t smin_moment_unit_bwd_ws_bytes(int N, int B, int L, int D);
int smin_moment_unit_bwd(void* stream, const float* dmu, const float* fcmean, const float* fb, const int32_t* cells,
                         const int32_t* row_ptr, const int32_t* cellmap, int N, int B, int L, int D, const float* WcatT,
                         float* dfcmean, float* dfb, float* dWcat, float* dbcat, void* ws, size_t ws_bytes,
                         int all_valid /* 1: every listed cell has m == 1 (mask-driven list): skips the mask lookups */,
                         const float* dfcmean_acc /* nullable [N][D]: added into dfcmean (a second consumer of fcmean) */,
                         const float* x1 /* nullable: the pair product saved by smin_moment_unit_fwd */,
                         const float* dfb_acc /* nullable [B][L][D]: added into dfb (another consumer's gradient of f_b) */);
/* The same three with the pair product stored as bf16 (uint16_t bit patterns, round to nearest even), x1h [N][D]: half the bytes of the
 * largest saved tensor of a layer.  Under smin_set_gemm_mode(2) -- where every contraction rounds its operands to bf16 as it loads them --
 * the results equal the fp32-storage calls bit for bit; in the other modes the product loses its low bits.  all_valid must be 1. */
int smin_pair_product_bf16(void* stream, const float* fb, const int32_t* cells, int N, int L, int D, uint16_t* x1h);
int smin_moment_unit_fwd_x1h(void* stream, const float* fcmean, const float* fm, const float* fb, const int32_t* cells,
                             int N, int B, int L, int D, const float* Wcat, const float* bcat, float* mu, const uint16_t* x1h);
int smin_moment_unit_bwd_x1h(void* stream, const float* dmu, const float* fcmean, const float* fb, const int32_t* cells,
                             const int32_t* row_ptr, const int32_t* cellmap, int N, int B, int L, int D, const float* WcatT,
                             float* dfcmean, float* dfb, float* dWcat, float* dbcat, void* ws, size_t ws_bytes,
                             int all_valid, const float* dfcmean_acc, const uint16_t* x1h, const float* dfb_acc);

/* ---- Localization.forward (models.py:335-344): score heads.
 *   pm [B][L][L] dense, zero-filled outside the cell list;  wb [3][D], bb [3] = (ps, pe, pa) heads;
 *   psea [3][B][L];  lmask [B][L] fp32 0/1. */
int smin_score_map_fwd(void* stream, const float* fm, const float* fb, const int32_t* cells, int N, int B, int L, int D,
                       const float* wm, const float* bm, const float* wb, const float* bb, const float* lmask,
                       float* pm, float* psea);
/* Forward-only tail of a scorer: the LAST layer's content-stream sum, its moment unit (models.py:288-303) and the map's score head
 * (models.py:337) multiplied out -- nobody but the score head reads the last mu.  With Wcat = [Wfb | Wfc] [D][2D], bcat = bias_fb + bias_fc,
 * Wc [D][dl], bc = content_unit.linear_c, wm, bm = conv_layer_pm:
 *   a = Wfb^T wm   c = Wfc^T wm   u = Wc^T c   k0 = bc.c + wm.bcat + bm
 *   pm[b,i,j] = sigmoid(sum_d a[d] bu[b,i,d] bu[b,j,d] + ccmean[n].u + (cumean[n] + hbar[n]).c + fm[n].wm + k0)   at the listed cells, 0 elsewhere
 * ccmean [N][dl] the attention core's clip-mean output, cumean [N][D] the clip mean entering the layer, hbar [N][D] the gate's output
 * (NULL: re-formed from fm and fs [B][D] as smin_gate_fwd does), fm [N][D] the layer's input, bu [B][L][D] its boundary output.
 * Writes what smin_score_map_fwd writes: pm dense [B][L][L], psea [3][B][L] (the same launch: bit-identical).  The list must be mask-driven
 * (every listed cell valid).  fp32 FMAs in every gemm mode; summation orders are fixed.  Requires D % 4 == 0, dl % 4 == 0, ws 16-byte
 * aligned with smin_score_tail_ws_bytes(B, L, D, dl) bytes.  Two stages that share nothing but ws (a, c, u, k0): the vectors, from
 * the parameters alone, and the cells.  pm == psea == NULL forms the vectors only; Wc == bc == Wcat == bcat == NULL scores the cells
 * with the vectors an earlier call left in ws (wm is read by both) -- so a host may form the vectors early, on another stream. */
size_t smin_score_tail_ws_bytes(int B, int L, int D, int dl);
int smin_score_tail_fwd(void* stream, const float* ccmean, const float* cumean, const float* hbar /* nullable */, const float* fm, const float* fs,
                        const float* bu, const int32_t* cells, int N, int B, int L, int D, int dl, const float* Wc, const float* bc,
                        const float* Wcat, const float* bcat, const float* wm, const float* bm, const float* wb /* [3][D] */,
                        const float* bb /* [3] */, const float* lmask, float* pm, float* psea, void* ws, size_t ws_bytes);
/* dpm [B][L][L], dpsea [3][B][L] -> dfm [N][D], dfb [B][L][D], dwm [D], dbm [1], dwb [3][D], dbb [3].  Two independent halves
 * (map score: dpm -> dfm, dwm, dbm; boundary heads: dpsea -> dfb, dwb, dbb): dpm == NULL or dpsea == NULL skips one (two streams).
 * ws_bytes >= smin_score_map_bwd_ws_bytes(N, B, L, D) (0 = arguments rejected: D % 4), which covers both halves. */
size_t smin_score_map_bwd_ws_bytes(int N, int B, int L, int D);
int smin_score_map_bwd(void* stream, const float* dpm, const float* dpsea, const float* pm, const float* psea,
                       const float* fm, const float* fb, const int32_t* cells, int N, int B, int L, int D,
                       const float* wm, const float* wb, const float* lmask,
                       float* dfm, float* dfb, float* dwm, float* dbm, float* dwb, float* dbb, void* ws, size_t ws_bytes);

/* ---- Restated train-step loss (reference main.py:89-116 with reduction='none'):
 *   loss = L_m + L_s + L_e + 0.5 L_a, scaled BCE, masked, per-sample mean then batch mean.
 * pm/sm [B][L][L], ps/pe/pa/ss/se [B][L] fp32; ym/mm [B][L][L], ys/ye/ya/lm [B][L] as bytes (bool / uint8).
 * loss [1]; part [B][6] scratch kept for backward.  Backward writes dpm [B][L][L], dps/dpe/dpa [B][L]. */
int smin_loss_fwd(void* stream, const float* pm, const uint8_t* ym, const float* sm, const uint8_t* mm,
                  const float* ps, const uint8_t* ys, const float* ss, const float* pe, const uint8_t* ye, const float* se,
                  const float* pa, const uint8_t* ya, const uint8_t* lm, int B, int L, float* loss, float* part);
int smin_loss_bwd(void* stream, const float* dloss, const float* part,
                  const float* pm, const uint8_t* ym, const float* sm, const uint8_t* mm,
                  const float* ps, const uint8_t* ys, const float* ss, const float* pe, const uint8_t* ye, const float* se,
                  const float* pa, const uint8_t* ya, const uint8_t* lm, int B, int L,
                  float* dpm, float* dps, float* dpe, float* dpa);

/* ---- masks and training targets of a batch (reference dataset.py:95-155: AbstractDataset.get_iou, get_boundary_penalties,
 * get_snippet_label and the mask construction of __getitem__, per sample on the host there).
 * times [B][2] = ground-truth (start, end) seconds, duration [B], nfeats [B] sampled frames (clamped to T), qlen [B] query
 * words.  Outputs (bytes are 0/1): video_mask [B][T], query_mask [B][Nq] (NULL with qlen NULL: not wanted), length_mask [B][L],
 * moment_mask [B][L][L], sm [B][L][L] fp32, ym, ss / se [B][L] fp32, ys, ye, ya.  Requires L | T. */
int smin_build_targets(void* stream, const float* times, const float* duration, const int32_t* nfeats, const int32_t* qlen, int B, int T, int L, int Nq,
                       uint8_t* video_mask, uint8_t* query_mask, uint8_t* length_mask, uint8_t* moment_mask, float* sm, uint8_t* ym,
                       float* ss, uint8_t* ys, float* se, uint8_t* ye, uint8_t* ya,
                       const float* two_sigma_sq /* [B] or NULL: 2 sigma^2 of the boundary Gaussians as computed in double from the unrounded
                                                    annotation times (dataset.py:116-119); NULL: formed in double from the fp32 times */);
/* masks only: with sm == NULL (and ym, ss, ys, se, ye, ya NULL as well) only video_mask, query_mask, length_mask and moment_mask are
 * written; times, duration and two_sigma_sq are not read and may be NULL. */

/* ---- clip resampling of raw per-video features (reference dataset.py:40-74, AbstractDataset.get_fixed_length_features, per
 * sample in numpy on the host there; csrc/sampling.hip).  raw [sum n_b][Din] (16-byte aligned), offsets [B+1] int64: sample b owns
 * rows offsets[b] .. offsets[b+1], n = their count.  Outputs video_features [B][T][Din], nfeats [B] = min(n, T).
 *   mode 0 (pick, the reference), in double: stride = 1 if n <= T else n / T; delta = (spos + stride) - spos (numpy arange's fill);
 *     row t < min(n, T) = raw row rint(spos + t * delta) of the sample (round half to even, np.round).  spos [B] or NULL (all 0, the
 *     eval split); a value outside the reference's draw range [0, int(r + 1)), r = stride - 0.5 minus 1 when integral
 *     (dataset.py:45-49), is clamped into it.
 *   mode 1 (mean; spos must be NULL): n <= T as pick; n > T: row t = mean of raw rows [a_t, a_{t+1}), a_t = rint(t * n / T) in double,
 *     a_T = n, summed in fp32 in ascending row order and divided once in fp32 by the row count (the 2D-TAN alternative the
 *     reference's comment at dataset.py:68-70 names).
 *   Rows t >= min(n, T) are zero (dataset.py:72-73).  Requires Din % 4 == 0, B <= 65535.  No host read; B = 0 is a no-op. */
int smin_sample_clips(void* stream, const float* raw, const int64_t* offsets, const int32_t* spos, int B, int T, int Din, int mode,
                      float* video_features, int32_t* nfeats);
/* its backward: dout [B][T][Din] -> draw [rows][Din] (rows = raw's row count), with the forward's offsets, spos and mode.  pick: a raw
 * row gets the sum of every dout[b, t] whose output row read it, added in ascending t (rows repeat once clipped at n - 1); mean: a raw
 * row gets dout[b, t] / cnt_t of its one window.  Rows no output row read (and rows outside every sample) are zero.  Deterministic
 * (no atomics); 16-byte aligned dout / draw. */
int smin_sample_clips_bwd(void* stream, const float* dout, const int64_t* offsets, const int32_t* spos, int B, int T, int Din, int mode,
                          int64_t rows, float* draw);
/* clip resampling of arbitrary row ranges (the windows of a long video): output sample w owns raw rows row_begin[w] ..
 * row_begin[w] + len[w] (int64 / int32 [W]; ranges may overlap and repeat, nothing is copied) and is exactly what smin_sample_clips
 * gives for a sample owning those rows with spos = 0, in either mode.  video_features [W][T][Din], nfeats [W] = min(len, T).  The
 * ranges must lie within raw (not checked).  Requires Din % 4 == 0, W <= 65535; no host read; W = 0 is a no-op. */
int smin_sample_windows(void* stream, const float* raw, const int64_t* row_begin, const int32_t* len, int W, int T, int Din, int mode,
                        float* video_features, int32_t* nfeats);

/* ---- query word vectors from token ids (reference dataset.py:32-38 get_query_features, dataset.py:173 query mask).
 * tokens [B][Nq] int32, table [V][E] (e.g. GloVe with <unk> and <pad> appended; 16-byte aligned, E % 4 == 0).
 * query_features [B][Nq][E] = table[tokens] (an id outside [0, V) gives a zero row), query_mask [B][Nq] = 0 <= id < pad_id
 * (bytes 0/1; an out-of-range id gives 0), qlen [B] = sum of the mask.  No host read; B = 0 is a no-op. */
int smin_embed_tokens(void* stream, const int32_t* tokens, const float* table, int B, int Nq, int V, int E, int pad_id,
                      float* query_features, uint8_t* query_mask, int32_t* qlen);
/* its backward: dqf [B][Nq][E] -> dtable [V][E] (dense, as nn.Embedding(sparse=False)): row v = sum of dqf[b, w] over the positions
 * holding id v, added in ascending (b, w) order; ids outside [0, V) contribute nothing; untouched rows are zero (the zero fill of the
 * whole table is part of the cost).  Deterministic (no atomics): the (id, position) pairs are sorted in one workgroup, then one
 * workgroup per distinct id.  Requires B * Nq <= 4096; ws of smin_embed_tokens_bwd_workspace_bytes (8-byte aligned). */
size_t smin_embed_tokens_bwd_workspace_bytes(int B, int Nq);
int smin_embed_tokens_bwd(void* stream, const int32_t* tokens, const float* dqf, int B, int Nq, int V, int E, float* dtable,
                          void* ws, size_t ws_bytes);
/* the same gradient as its distinct rows (csrc/row_sparse.hip), for a table too large to sweep: with n = B * Nq <= 4096,
 * ids [n] int32, rows [n][E], count [1] int32, sqnorm [1] double.  Slots s < count hold the distinct ids in [0, V) in strictly ascending
 * order; rows[s] = sum of dqf[b, w] over the positions holding ids[s], added in ascending (b, w) order -- the additions of the dense
 * entry above, so rows[s] has the bits of dtable[ids[s]].  Slots s >= count get ids[s] = -1 and their rows are not written.  sqnorm = the
 * sum of squares of the count rows, accumulated in double in a fixed order.  B = 0 or no id in range gives count = 0, sqnorm = 0.
 * Deterministic (no atomics); three launches sized by n that exit early on the device-side count: no host read, no pass over V * E.
 * Requires 16-byte aligned dqf / rows, E % 4 == 0; ws of the query below (8-byte aligned). */
size_t smin_embed_tokens_bwd_rows_workspace_bytes(int B, int Nq);
int smin_embed_tokens_bwd_rows(void* stream, const int32_t* tokens, const float* dqf, int B, int Nq, int V, int E, int32_t* ids, float* rows,
                               int32_t* count, double* sqnorm, void* ws, size_t ws_bytes);

/* ---- compute_ious (reference utils.py:10-31): counts [8] = number of samples with a hit for
 * R@1 x IoU {0.1, 0.3, 0.5, 0.7} then R@5 x the same; ws [B][8] scratch.  Any L with L*L >= 5 (the reference's topk(5) needs as many). */
int smin_compute_ious(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                      int B, int L, float* counts, float* ws);

/* ---- top-k moments with greedy temporal NMS (csrc/moments.hip).  For each sample b:
 *   candidates: cells (i, j) with mm[b,i,j] != 0 (masked cells are never returned);
 *   score = (pm[b,i,j] * sqrtf(ps[b,i])) * sqrtf(pe[b,j]) in fp32, in this order, correctly rounded sqrtf;
 *   order: higher score first, ties -> lower flat index i*L + j (a score of -0 counts as +0);
 *   IoU of two cells (moment (i, j) spans clips [i, j+1)): inter = max(0, min(j1,j2) + 1 - max(i1,i2)),
 *     union = max(j1,j2) + 1 - min(i1,i2), iou = (float)inter / (float)union (one correctly rounded division);
 *   greedy NMS: walk the candidates in order, keep one unless its IoU with a kept cell is > nms_thresh; stop after k kept or
 *     when the candidates run out.  nms_thresh >= 1: no suppression (plain top-k over the valid cells).
 * Outputs: idx [B][k][2] (start clip i, end clip j; -1 for empty slots), score [B][k] (0 for empty slots), count [B] (kept).
 * Limits: 1 <= k <= 64, 1 <= B <= 65535 (the sample is the y coordinate of the band select's grid), L >= 1, L*L < 2^31; the same
 * holds for smin_compute_ious_nms and rule 1 of the epoch meter below, which run these launches.  The result is exact and
 * independent of the internal candidate buffers; fp32 subnormal scores are kept (no flush to zero) and ordered like any other.
 * No host synchronisation (capturable in a HIP graph).  ws: device scratch of at least the _ws_bytes size (0 = arguments rejected). */
size_t smin_top_moments_ws_bytes(int B, int L, int k);
int smin_top_moments(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k,
                     float nms_thresh, long long* idx, float* score, int* count, void* ws, size_t ws_bytes);

/* ---- merge of per-window top-k moments across the windows of a long video (csrc/moments.hip; SMIN.localize_windows).
 * Inputs: smin_top_moments' outputs of G windows at k_window: idx [G][k_window][2] int64, score [G][k_window], count [G]; each
 * window's first raw row start [G] int64 (relative to its video) and row count len [G] int32; pair_ptr [B+1] int64: pair b owns
 * windows pair_ptr[b] .. pair_ptr[b+1] (ordinal g - pair_ptr[b] within the pair).  All arithmetic fp32, in this order:
 *   span of kept cell (i, j) of window (s, len), in raw rows:  u = (float)max(len, T) / (float)L;  st = (float)s + (float)i * u;
 *     en = fminf((float)s + (float)(j + 1) * u, (float)(s + len))   (each operation rounded once, no contraction);
 *   candidates of pair b: the first count[g] slots of each of its windows;
 *   order: higher score first (-0 equals +0), ties -> lower window ordinal, then lower slot;
 *   IoU of two spans: inter = fmaxf(0, fminf(en1, en2) - fmaxf(st1, st2)), uni = fmaxf(en1, en2) - fminf(st1, st2),
 *     iou = inter / uni (one correctly rounded division);
 *   greedy NMS: walk the candidates in order, keep one unless its IoU with a kept one is > nms_thresh; stop after k kept.
 *     nms_thresh >= 1: no suppression.
 * Outputs: span [B][k][2] fp32 (NaN for empty slots), out_score [B][k] (the candidate's score; 0), window [B][k] int64 (ordinal
 * within the pair; -1), cell [B][k][2] int64 ((i, j); -1), out_count [B] (kept).
 * Limits: 1 <= k, k_window <= 64, G * k_window < 2^31, T >= 1, L >= 1 (else a negative code, nothing launched); B = 0 is a no-op;
 * pointers may be NULL only for B = 0 (inputs: for G = 0).  Deterministic, no scratch, no host synchronisation. */
int smin_merge_window_moments(void* stream, const int64_t* idx, const float* score, const int32_t* count, const int64_t* start,
                              const int32_t* len, const int64_t* pair_ptr, int G, int B, int T, int L, int k_window, int k,
                              float nms_thresh, float* span, float* out_score, int64_t* window, int64_t* cell, int32_t* out_count);

/* ---- R@n, IoU=m over the NMS-kept moments: the top-k moments above with k = max(n_list), then for each pair (a, c)
 * counts[a * nm + c] = number of samples with sm[b] > m_list[c] at any of the first n_list[a] kept cells (an empty slot
 * counts as IoU 0).  1 <= n_list[a] <= k, 1 <= nn <= 64, 1 <= nm <= 16; host arrays n_list / m_list; deterministic sum
 * over the samples.  ws: device scratch of at least the _ws_bytes size. */
size_t smin_compute_ious_nms_ws_bytes(int B, int L, int k, int nn, int nm);
int smin_compute_ious_nms(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                          int B, int L, int k, float nms_thresh, const int* n_list, int nn, const float* m_list, int nm,
                          float* counts, void* ws, size_t ws_bytes);

/* ---- epoch meter (csrc/metrics.hip): the two metrics above, accumulated over the batches of an epoch in device memory, with no
 * host read per batch.  acc [4 + nn * nm] doubles, zeroed by the caller before the first update:
 *   [0] samples seen;  [1] sum of (double)loss[0] * B over the updates that passed a loss;  [2] samples of those updates;
 *   [3] sum of the top-1 IoU;  [4 + a * nm + c] samples with a hit for (n_list[a], m_list[c]).
 * rule 0: the reference's rule, exactly smin_compute_ious (score times mask, top five of all L*L cells); accepted only with
 *   k = 5, n_list = {1, 5}, m_list = {0.1f, 0.3f, 0.5f, 0.7f} and L*L >= 5; nms_thresh is not read.
 * rule 1: valid cells with greedy temporal NMS, exactly smin_compute_ious_nms (k >= max(n_list), k <= 64, nn <= 64, nm <= 16;
 *   nms_thresh >= 1: plain top-k).
 * Top-1 IoU of a sample, both rules: sm at its first kept cell, 0 if it keeps none.
 * Arithmetic: the per-sample stage is the one of the two entry points above (one workgroup per sample; fp32 hit flags 0 / 1 and the
 * top-1 IoU per sample in ws).  One closing wave then forms, for each slot, s = 0.0; for b = 0 .. B-1: s += (double)x[b]; and adds
 * acc[slot] += s (slots 0 and 2: x[b] = 1); the loss slot is acc[1] += (double)loss[0] * (double)B.  loss: device [1] or NULL (then
 * slots 1 and 2 stay).  No atomics, no host read: everything is ordered by the stream, so ALL UPDATES OF ONE acc MUST BE ISSUED ON
 * ONE STREAM (or be ordered by events), and a reader of acc must be ordered behind the last update.  n_list / m_list: host arrays.
 * _ws_bytes returns 0 when the arguments are rejected. */
size_t smin_epoch_meter_ws_bytes(int B, int L, int rule, int k, int nn, int nm);
int smin_epoch_meter_update(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                            int B, int L, int rule, int k, float nms_thresh, const int* n_list, int nn, const float* m_list, int nm,
                            const float* loss, double* acc, void* ws, size_t ws_bytes);

/* ---- Soft-NMS moment retrieval (csrc/soft_nms.hip): top-k where a pick decays the candidates it overlaps instead of removing them,
 * and the rest is ranked again.  Candidates, score, IoU, order (ties -> lower flat index, -0 counts as +0), empty slots and the limits
 * on B, L and k are smin_top_moments' above.  Per sample, with cur(c) = score(c) initially:
 *   pick:   the remaining candidate with the highest cur (order word of cur, then the lower flat index);
 *   stop:   after k picks, when no candidate is left, or when the best cur < min_score (fp32; -inf never stops early);
 *   record: idx, score = cur at pick time, raw_score = the picked cell's undecayed score (a zero is written as +0);
 *   decay:  for every remaining candidate iou with the pick (one correctly rounded fp32 division), then cur = cur * w, one fp32
 *           multiplication, no fma contraction:
 *             method SMIN_NMS_LINEAR:    w = iou > nms_thresh ? 1.0f - iou : 1.0f      (sigma is not read)
 *             method SMIN_NMS_GAUSSIAN:  w = expf(-(iou * iou) / sigma), every candidate; sigma > 0, +inf allowed (w = 1);
 *                                        nms_thresh is not read
 * The decays are applied in pick order, cur = ((s0 * w1) * w2) ...; the result does not depend on how the work is split.  The linear
 * rule is made of correctly rounded fp32 operations and is reproducible bit for bit; the gaussian rule is as exact as the device
 * library's expf.  With linear and nms_thresh >= 1, or gaussian and sigma = +inf, the lists are smin_top_moments' at nms_thresh >= 1.
 * Signed scores follow the same formulas.  NaN and +-inf at VALID cells are out of scope for the soft rules; NaN and inf at masked
 * cells are never read into the order.
 * Worked example (L = 4, ps = pe = 1, valid cells (0,3) = 1.0, (0,2) = 0.9f, (3,3) = 0.5, every other valid cell 0; linear,
 * nms_thresh = 0.5, k = 3): pick (0,3) at 1.0; (0,2) has IoU 3/4 with it and becomes 0.9f * 0.25f; (3,3) has IoU 1/4 and stays 0.5;
 * the picks are (0,3), (3,3), (0,2) with scores 1.0, 0.5, 0.9f * 0.25f.  Plain top-k gives (0,3), (0,2), (3,3); hard NMS at 0.5 drops
 * (0,2) and gives (0,3), (3,3) and a cell of score 0.
 * Outputs: idx [B][k][2] (-1), score [B][k] (0), raw_score [B][k] (0), count [B].
 * Launches: maps with L*L <= 12288 cells take one launch (one workgroup per sample, cur in LDS); larger maps take k + 1 launches over
 * a band grid with cur in ws.  No workgroup waits on another, no float atomics, no host read: the same bits on every run, capturable
 * in a HIP graph.  ws: device scratch of at least the _ws_bytes size; the query returns 0 when (B, L, k) are rejected, and 256 (unused)
 * on the one-launch path.  A bad method, sigma <= 0 or NaN (gaussian), a NULL pointer or a short ws: a negative code, nothing launched. */
#define SMIN_NMS_LINEAR 1
#define SMIN_NMS_GAUSSIAN 2
size_t smin_top_moments_soft_ws_bytes(int B, int L, int k);
int smin_top_moments_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k,
                          int method, float nms_thresh, float sigma, float min_score, long long* idx, float* score, float* raw_score,
                          int* count, void* ws, size_t ws_bytes);
/* the span form: smin_merge_window_moments' inputs, candidates, order, spans and span IoU, with the soft rule above in place of the
 * threshold.  cur starts at the candidate's input score; out_score = cur at pick time, raw_score = the input score (both as they
 * are, no sign change).  The caller passes UNDECAYED per-window scores (smin_top_moments_soft's raw_score): the merge decays once, in
 * raw-row time.  One workgroup per pair, every round recomputes cur from the kept spans in pick order: no scratch. */
int smin_merge_window_moments_soft(void* stream, const int64_t* idx, const float* score, const int32_t* count, const int64_t* start,
                                   const int32_t* len, const int64_t* pair_ptr, int G, int B, int T, int L, int k_window, int k,
                                   int method, float nms_thresh, float sigma, float min_score, float* span, float* out_score,
                                   float* raw_score, int64_t* window, int64_t* cell, int32_t* out_count);
/* smin_compute_ious_nms and rule 1 of the epoch meter with the soft selection (min_score = -inf) in place of the greedy hard NMS: the
 * same hit flags, sums and closing wave behind it.  Same limits and rejections as above. */
size_t smin_compute_ious_soft_ws_bytes(int B, int L, int k, int nn, int nm);
int smin_compute_ious_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                           int B, int L, int k, int method, float nms_thresh, float sigma, const int* n_list, int nn,
                           const float* m_list, int nm, float* counts, void* ws, size_t ws_bytes);
size_t smin_epoch_meter_soft_ws_bytes(int B, int L, int k, int nn, int nm);
int smin_epoch_meter_update_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                 int B, int L, int k, int method, float nms_thresh, float sigma, const int* n_list, int nn,
                                 const float* m_list, int nm, const float* loss, double* acc, void* ws, size_t ws_bytes);

/* ---- span metric (csrc/metrics.hip): IoU, R@n, IoU=m and top-1 IoU of continuous spans -- smin_merge_window_moments' output --
 * against one ground-truth span per pair, and their accumulation into the epoch meter's acc.
 * Inputs: span [B][k][2] fp32 (st, en) and count [B] (slots s >= count[b] are empty; their span, NaN, is never used), gt [B][2]
 * fp32 (gs, ge) in the same unit (raw rows of the pair's video, as the merge returns them; seconds work equally).
 * All arithmetic fp32, in this order, each operation rounded once:
 *   IoU of slot s < count[b]:  inter = fmaxf(0, fminf(en, ge) - fmaxf(st, gs));  uni = fmaxf(en, ge) - fminf(st, gs);
 *     iou = uni > 0 ? inter / uni : 0   (one correctly rounded division; the operation order of the merge's IoU);
 *   a slot s >= count[b] has IoU exactly 0 (the rule of smin_compute_ious_nms: an empty slot counts as IoU 0);
 *   count[b] is read clamped to [0, k] by both entry points: a negative count is 0 filled slots, a count above k is k;
 *   hit for (n_list[a], m_list[c]): some slot s < min(n_list[a], count[b]) with iou > m_list[c] (strict);
 *   top-1 IoU: the IoU of slot 0, 0 when count[b] == 0.
 * smin_span_ious writes iou [B][k].  smin_span_meter_update adds to acc [4 + nn * nm] doubles, the accumulator of
 * smin_epoch_meter_update with the same slots: [0] += B, [3] += the sum of the top-1 IoU, [4 + a * nm + c] += the hits; [1] and [2]
 * are not touched.  The per-pair stage (one lane per pair; fp32 hit flags 0 / 1 and the top-1 IoU in ws) is followed by the
 * meter's closing wave: s = 0.0; for b = 0 .. B-1: s += (double)x[b]; acc[slot] += s.  No atomics, no host read: ALL UPDATES OF
 * ONE acc, of either kind, MUST BE ISSUED ON ONE STREAM (or be ordered by events).  n_list / m_list: host arrays.
 * Limits: 1 <= k <= 64, 1 <= nn <= 64, 1 <= nm <= 16, every n_list[a] in [1, k], B >= 0 (else a negative code, nothing launched);
 * B = 0 is a no-op.  ws: device scratch of at least the _ws_bytes size; _ws_bytes returns 0 when B < 1 or nn / nm are rejected. */
int smin_span_ious(void* stream, const float* span, const int32_t* count, const float* gt, int B, int k, float* iou);
size_t smin_span_meter_ws_bytes(int B, int nn, int nm);
int smin_span_meter_update(void* stream, const float* span, const int32_t* count, const float* gt, int B, int k,
                           const int* n_list, int nn, const float* m_list, int nm, double* acc, void* ws, size_t ws_bytes);

/* ---- corpus metric (csrc/metrics.hip): video-corpus moment retrieval (VCMR) recall R@n, IoU=m, video retrieval
 * (VR) recall R@n and the top-1 IoU of ranked lists over a corpus -- SMIN.search / smin_search_merge output -- against one ground-truth
 * moment of one ground-truth video per query, accumulated as the span metric accumulates.
 * Inputs: video [Q][k] int64, span [Q][k][2] fp32 (st, en), count [Q] int32 (read clamped to [0, k]; entries r >= count[q] are empty
 * and never read), gt_video [Q] int64, gt [Q][2] fp32 (gs, ge) in span's unit: seconds, or clip edges (i, j + 1).
 * Per query, over the entries r < cnt = clamp(count[q], 0, k):
 *   iou[r] = the span metric's IoU of span[r] with gt (fp32, each operation rounded once) if video[r] == gt_video[q], else 0;
 *   top-1 IoU: iou[0], 0 when cnt == 0;
 *   VCMR hit for (n_list[a], m_list[c]): some r < min(n_list[a], cnt) with iou[r] > m_list[c] (strict);
 *   VR hit for n_list[a]: some entry has video[r] == gt_video[q] and, for the first such r, the number of distinct videos among the
 *     entries 0 .. r-1 is < n_list[a] (the ground-truth video is among the first n distinct videos of the list);
 *   a query whose ground-truth video is not listed is a miss everywhere.
 * acc [4 + nn * nm + nn] doubles: [0] += Q, [1] and [2] are not touched, [3] += the sum of the top-1 IoU, [4 + a * nm + c] += the VCMR
 * hits, [4 + nn * nm + a] += the VR hits; every sum is s = 0.0; for q = 0 .. Q-1: s += (double)x[q]; acc[slot] += s (the epoch
 * meter's closing wave over nn * nm + nn slots).  No atomics, no host read: ALL UPDATES OF ONE acc MUST BE ISSUED ON ONE STREAM.
 * Limits: 1 <= k <= 64, 1 <= nn <= 64, 1 <= nm <= 16, every n_list[a] in [1, k], Q >= 0 (else a negative code, nothing launched);
 * Q = 0 is a no-op.  n_list / m_list: host arrays.  ws: device scratch of at least the _ws_bytes size (0: Q < 1 or nn / nm rejected). */
size_t smin_corpus_meter_ws_bytes(int Q, int nn, int nm);
int smin_corpus_meter_update(void* stream, const int64_t* video, const float* span, const int32_t* count, const int64_t* gt_video,
                             const float* gt, int Q, int k, const int* n_list, int nn, const float* m_list, int nm, double* acc,
                             void* ws, size_t ws_bytes);

/* ---- content stream (reference models.py:242-276 + 115-119, re-associated): the content unit's output
 *   f_c' = m*(cc Wc^T + bc) + f_c + hbar   (models.py:269-276)
 * is consumed only by the next unit's linear_c_hat (models.py:247) and, through mean_c, by the moment unit
 * (models.py:295).  Both are linear, so the (N*C) x D tensor f_c is never formed: with g = f Wch^T,
 *   chat_k = window_mean(g_k) + sum_{l<k} cc_l (Wch_k Wc_l)^T + (sum_{l<k} hbar_l) Wch_k^T + const
 *   mean_c f_c^k = mean_c f_c^{k-1} + (mean_c cc_k) Wc_k^T + bc_k + hbar_k
 * and every contraction over N*C rows has K, N <= dl.  The entry points below are the pieces; the Python host
 * (modules.py: SMIN.forward) composes them under autograd.  Requires a mask-driven cell list (m == 1 everywhere). */

/* out[s][n*C + c][:] = m * (mean over clip c of cell n of g[b][t][s*W:(s+1)*W] + bias[s*W:(s+1)*W])
 * g [B][T][nseg*W] (nseg <= 8: one segment per layer), out [nseg][N*C][W];
 * ws_bytes >= smin_clip_window_means_fwd_ws_bytes(B, T, W, nseg) (0 = arguments rejected: W % 4, nseg outside 1..8, nseg*W > 2048). */
size_t smin_clip_window_means_fwd_ws_bytes(int B, int T, int W, int nseg);
int smin_clip_window_means_fwd(void* stream, const float* g, const float* bias /* [bias_len], first features only */, int bias_len,
                               const int32_t* cells, int N, int B, int T, int L, int C,
                               int W, int nseg, float* out, void* ws, size_t ws_bytes);
/* dout: HOST array of nseg device pointers, dout[s] [N*C][W] -> dg [B][T][nseg*W];
 * ws_bytes >= smin_clip_window_means_bwd_ws_bytes(B, T, W, nseg) (0 = rejected, as above); neither read nor checked when N == 0. */
size_t smin_clip_window_means_bwd_ws_bytes(int B, int T, int W, int nseg);
int smin_clip_window_means_bwd(void* stream, const float* const* dout, const int32_t* cells, const int32_t* row_ptr,
                               const int32_t* cellmap, int N, int B, int T, int L, int C, int W, int nseg, float* dg,
                               void* ws, size_t ws_bytes, const int32_t* ev_offsets, const void* ev_table);

/* attention core of the content unit alone (models.py:252-267): chat [N*C][dl] -> cc [N*C][dl] and/or ccmean [N][dl]
 * (either output may be NULL). */
int smin_content_attn_fwd(void* stream, const float* chat, const int32_t* cells, const int32_t* row_ptr,
                          int N, int B, int L, int C, int dl, int Nq,
                          const float* Mq, const float* uq, const float* what, const float* shat, const float* qmask,
                          float* cc, float* ccmean);
/* smin_content_attn_fwd with the rows stored as bf16 (cc_h [N*C][dl], round to nearest even) beside the fp32 clip mean */
int smin_content_attn_fwd_cch(void* stream, const float* chat, const int32_t* cells, const int32_t* row_ptr,
                              int N, int B, int L, int C, int dl, int Nq,
                              const float* Mq, const float* uq, const float* what, const float* shat, const float* qmask,
                              uint16_t* cc_h, float* ccmean);
/* smin_content_attn_fwd that also stores the word probabilities of every packed row, ContentAttention.attn_weights
 * (models.py:207-226): probs [N*C][Nq] fp32, padded words exactly 0.  cc may be NULL (no rows), fp32 [N*C][dl], or, with
 * cc_bf16 != 0, bf16 [N*C][dl] (then ccmean is required).  cc / ccmean are bit-identical to smin_content_attn_fwd(_cch). */
int smin_content_attn_fwd_probs(void* stream, const float* chat, const int32_t* cells, const int32_t* row_ptr,
                                int N, int B, int L, int C, int dl, int Nq,
                                const float* Mq, const float* uq, const float* what, const float* shat, const float* qmask,
                                void* cc, int cc_bf16, float* ccmean, float* probs);
/* Dense ContentAttention.attn_weights out [B][L][L][C][Nq] (models.py:207-226) from packed probs [N*C][Nq]: a cell with
 * cellmap[b][i][j] = n >= 0 and m = cells[n][3] != 0 copies rows n*C .. n*C+C-1; any other cell gets the reference's value
 * there, softmax over words of mask(uq[b] / sqrt(dl)) (its c_hat is 0, so its query is W_q.bias; uq from smin_word_prep_fwd). */
int smin_content_attn_maps_dense(void* stream, const float* probs, const int32_t* cellmap, const int32_t* cells,
                                 int B, int L, int C, int dl, int Nq, const float* uq, const float* qmask, float* out);
/* The maps of the moments top_moments kept (idx [B][k][2] int64 start / end, -1 = empty slot), without a dense map:
 * probs / bmaps are HOST arrays of nl <= SMIN_ATTN_MAPS_MAX_LAYERS device pointers, probs[l] [N*C][Nq] (content, models.py:207-226)
 * and bmaps[l] [B][L][Nq] (boundary, Attention.attn_weights, models.py:137-154).  content [B][k][nl][C][Nq] = probs[l] rows of the
 * cell cellmap[b][i][j]; boundary [B][k][nl][2][Nq] = bmaps[l] rows i and j.  Empty slots are 0. */
#define SMIN_ATTN_MAPS_MAX_LAYERS 8
int smin_attn_maps_gather(void* stream, const float* const* probs, const float* const* bmaps, int nl, const int32_t* cellmap,
                          const int64_t* idx, int B, int L, int C, int Nq, int k, float* content, float* boundary);
size_t smin_content_attn_bwd_workspace_bytes(int N, int B, int C, int dl);
/* dcc [N*C][dl] and/or dccmean [N][dl] (one may be NULL) -> dchat [N*C][dl], dMq, duq, dwhat, dshat. */
int smin_content_attn_bwd(void* stream, const float* dcc, const float* dccmean, const float* chat,
                          const int32_t* cells, const int32_t* row_ptr, int N, int B, int L, int C, int dl, int Nq,
                          const float* Mq, const float* uq, const float* what, const float* shat, const float* qmask,
                          float* dchat, float* dMq, float* duq, float* dwhat, float* dshat, void* ws, size_t ws_bytes);

/* y[r][:] = [x_0[r] | .. | x_{nseg-1}[r]] W^T + bias + add_rows[r][:] + add_cells[r / C][:]
 * xs: HOST array of nseg <= 4 device pointers, x_s [R][K]; W [O][nseg*K]; y [R][O]; bias, add_rows, add_cells may
 * be NULL.  Backward: dx_s = dy W_s (dxs: HOST array of nseg device pointers, or NULL; WT = W^T [nseg*K][O]),
 * dW [O][nseg*K] = dy^T [x_0 | ..] (NULL, with dbias NULL, to skip the weight half), dbias = colsum(dy) (may be NULL);
 * the gradient of add_rows is dy itself, of add_cells smin_group_sum(dy). */
int smin_linear_rows_fwd(void* stream, const float* const* xs, int nseg, const float* W, const float* bias, const float* add_rows,
                         const float* add_cells, int C, int R, int O, int K, float* y);
size_t smin_linear_rows_bwd_workspace_bytes(int R, int O, int Ktot);
int smin_linear_rows_bwd(void* stream, const float* dy, const float* const* xs, int nseg, const float* WT, int R, int O, int K,
                         float* const* dxs, float* dW, float* dbias, void* ws, size_t ws_bytes);
/* smin_linear_rows_fwd / the weights half of smin_linear_rows_bwd for xs stored as bf16 (uint16_t bit patterns; contraction-only operands
 * under smin_set_gemm_mode(2), where the results equal the fp32-storage calls bit for bit).  Forward: add_rows and add_cells required. */
int smin_linear_rows_fwd_xh(void* stream, const uint16_t* const* xs, int nseg, const float* W, const float* bias, const float* add_rows,
                            const float* add_cells, int C, int R, int O, int K, float* y);
int smin_linear_rows_bwd_xh(void* stream, const float* dy, const uint16_t* const* xs, int nseg, int R, int O, int K,
                            float* dW, float* dbias, void* ws, size_t ws_bytes);
/* dx_s += dy W_s for every segment (WT as above): input gradients accumulated into tensors that already hold another consumer's gradient */
int smin_linear_rows_dx_acc(void* stream, const float* dy, int nseg, const float* WT, int R, int O, int K, float* const* dxs);
/* out[g][:] = sum_{c<C} x[g*C + c][:]   (x [groups*C][W]) */
int smin_group_sum(void* stream, const float* x, int groups, int C, int W, float* out);

/* ---- word-side operands of every layer's content attention in one launch (ContentUnit.forward models.py:249-251 and the
 * word half of ContentAttention.forward models.py:209-211, with W_q folded onto the words).  Per layer k:
 *   what_k = (f_w WH_k^T + bWH_k) * qmask,  shat_k = f_s SH_k^T + bSH_k,  kb_k = what_k AK_k^T + bAK_k,  Mq_k = kb_k AQ_k,  uq_k = kb_k . bAQ_k
 * params: HOST array of nl*8 device pointers, per layer [WH (dl,D), bWH, SH (dl,D), bSH, AK (dl,dl), bAK, AQ (dl,dl), bAQ]
 * (= linear_w_hat, linear_s_hat, attn_layer.W_k, attn_layer.W_q).  fw [B][Nq][D], fs [B][D], qmask [B][Nq] fp32.
 * Outputs, layer-major: what, kb, Mq [nl][B][Nq][dl], shat [nl][B][dl], uq [nl][B][Nq].  nl <= 8, Nq <= 32, dl <= 128. */
int smin_word_prep_fwd(void* stream, const float* fw, const float* fs, const float* qmask, const float* const* params, int nl, int B, int Nq, int D,
                       int dl, float* what, float* shat, float* kb, float* Mq, float* uq);
size_t smin_word_prep_bwd_workspace_bytes(int nl, int B, int Nq, int D, int dl);
/* dwhat / dshat / dMq / duq: HOST arrays of nl device pointers (per-layer gradients [B][..]; NULL entries = zero).
 * -> dfw [B][Nq][D], dfs [B][D], dparams: HOST array of nl*8 device pointers (same order as params), all written. */
int smin_word_prep_bwd(void* stream, const float* const* dwhat, const float* const* dshat, const float* const* dMq, const float* const* duq,
                       const float* fw, const float* fs, const float* qmask, const float* what, const float* kb, const float* const* params,
                       int nl, int B, int Nq, int D, int dl, float* dfw, float* dfs, float* const* dparams, void* ws, size_t ws_bytes);

/* ---- VideoEncoder (models.py:25-36) fused with the backbone's Hadamard product (models.py:81-83):
 *   fv[b][t][:] = (x[b][t][:] W^T + bias + pe[t][:]) * vmask[b][t]     f[b][t][:] = fv[b][t][:] * fs[b][:]
 * x [B*T][Din], W [D][Din], pe [>=T][D] (rows 0..T-1 are used), vmask [B*T] fp32, fs [B][D]; outputs fv, f [B*T][D].
 * fs == f == NULL: the projection alone (fv); smin_video_encoder_gate then forms f = fv * fs -- a host can run the projection
 * beside the query encoder (which produces fs) and pay only the product behind it. */
int smin_video_encoder_fwd(void* stream, const float* x, const float* W, const float* bias, const float* pe, const float* vmask,
                           const float* fs, int B, int T, int Din, int D, float* fv, float* f);
int smin_video_encoder_gate(void* stream, const float* fv, const float* fs, int B, int T, int D, float* f);
size_t smin_video_encoder_bwd_workspace_bytes(int B, int T, int Din, int D);
/* df [B*T][D] -> dW [D][Din], dbias [D], dpe [T][D], dfs [B][D].  May be issued as two calls on the same ws (e.g. on two streams, the
 * second ordered behind the first): dW == NULL -> inputs half (dfs; the masked gradient stays in ws); df == NULL -> weights half. */
int smin_video_encoder_bwd(void* stream, const float* df, const float* fv, const float* fs, const float* vmask, const float* x,
                           int B, int T, int Din, int D, float* dW, float* dbias, float* dpe, float* dfs, void* ws, size_t ws_bytes);
/* the input feature's gradient dx [B*T][Din] = dv W, dv = df * fs * vmask the masked gradient that the inputs half above left in ws
 * (the same ws; issue it behind that half, before or beside the weights half, which only reads ws as well).  WT = W^T [Din][D].
 * Rows of padded frames (vmask = 0) are exactly zero.  Requires Din % 4 == 0, D % 4 == 0. */
int smin_video_encoder_bwd_input(void* stream, const float* WT, const float* vmask, int B, int T, int Din, int D, float* dx,
                                 const void* ws, size_t ws_bytes);

/* ---- QueryEncoder's bidirectional LSTM layer (models.py:38-64: nn.LSTM over a packed, padded batch), one layer per
 * call, both directions.  X [B*Nq][In]; Wih_cat [8H][In] = [W_ih; W_ih_reverse]; bias_cat [8H] = b_ih + b_hh per
 * direction; W4 [2][H][H][4] with W4[d][k][u][g] = W_hh_d[g*H+u][k]; len [B] valid lengths (device).  Outputs: Hout
 * [B][Nq][2H] (zero at padded positions, as pad_packed_sequence gives), and for backward G [B][Nq][2][4H] (gate
 * activations i,f,g,o) and Cs [B][Nq][2][H] (cell states).  Requires In % 4 == 0, H % 4 == 0, H <= 256. */
/* sentence feature (models.py:60-62): fs [B][2H], fs[b] = [fw[b][len_b - 1][0:H] | fw[b][0][H:2H]] with fw [B][Nq][2H] (len clamped to
 * 1..Nq); backward adds dfs into the same entries of dfw (in place) */
int smin_sentence_feature_fwd(void* stream, const float* fw, const int32_t* len, int B, int Nq, int H, float* fs);
int smin_sentence_feature_bwd(void* stream, const float* dfs, const int32_t* len, int B, int Nq, int H, float* dfw);
/* the operand layouts above from nn.LSTM's eight parameter tensors of a layer (w: HOST array of 8 device pointers: weight_ih, weight_hh,
 * bias_ih, bias_hh of the forward direction, then of the reverse direction), one launch; also writes Whh [2][4H][H] for the backward call */
int smin_lstm_pack(void* stream, const float* const* w, int In, int H, float* Wih, float* bias, float* Whh, float* W4);
/* every layer of the encoder (nlayers <= 4) in one launch, ahead of the first recurrence: w = HOST array of 8 * nlayers device pointers
 * (layer by layer, each in smin_lstm_pack's order), In = HOST array of the layers' input widths, outputs = HOST arrays of nlayers pointers */
int smin_lstm_pack_layers(void* stream, int nlayers, const float* const* w, const int* In, int H, float* const* Wih, float* const* bias,
                          float* const* Whh, float* const* W4);
int smin_bilstm_layer_fwd(void* stream, const float* X, const float* Wih_cat, const float* bias_cat, const float* W4,
                          const int32_t* len, int B, int Nq, int In, int H, float* G, float* Hout, float* Cs);
size_t smin_bilstm_layer_bwd_workspace_bytes(int B, int Nq, int In, int H);
/* dHout [B][Nq][2H] -> dX [B*Nq][In] (NULL to skip), dWih_cat [8H][In], dbias_cat [8H] (= d b_ih = d b_hh),
 * dWhh [2][4H][H].  Wih_catT [In][8H]; Whh [2][4H][H] (W_hh per direction, as nn.LSTM stores it).  May be issued as two calls on the
 * same ws: dWih_cat == NULL -> inputs half (the recurrence and dX; gate gradients stay in ws); dHout == NULL -> weights half. */
int smin_bilstm_layer_bwd(void* stream, const float* dHout, const float* X, const float* Hout, const float* G, const float* Cs,
                          const float* Wih_catT, const float* Whh, const int32_t* len, int B, int Nq, int In, int H,
                          float* dX, float* dWih_cat, float* dbias_cat, float* dWhh, void* ws, size_t ws_bytes);
/* The weights half in up to three independent pieces, each with its own part of ws (which: bit 0 = dWih_cat + dbias_cat, bit 1 =
 * dWhh[0], bit 2 = dWhh[1]; 7 = what smin_bilstm_layer_bwd's weights half does): pieces issued on different streams run side by
 * side behind the inputs half (they are the last kernels of a train step, models.py:46-62 backward).
 * dbias_cat2 (NULL to skip): a second copy of dbias_cat -- b_ih and b_hh have the same gradient and each needs memory of its own. */
int smin_bilstm_layer_bwd_weights(void* stream, int which, const float* X, const float* Hout, int B, int Nq, int In, int H,
                                  float* dWih_cat, float* dbias_cat, float* dbias_cat2, float* dWhh, void* ws, size_t ws_bytes);

/* The recurrences above run, for H a multiple of 32, as clusters of workgroups that keep W_hh in LDS and exchange h / dh through
 * tagged granules in global memory (csrc/bilstm_cluster.hip); every poll there is bounded.  Returns 1 once a poll has expired since
 * the last call (the launch that hit it produced wrong values), 0 otherwise; clears the word.  Synchronises the device. */
int smin_lstm_cluster_error(void);

/* ---- packed valid-cell layout from a (B, L, L) mask (uint8 / bool, non-zero = valid).  all_cells = 0: list the valid
 * cells (m = 1); 1: list every (b, i, j) with m = mask.  cells [N][4] = {b, i, j, m} sorted by (b, i, j); row_ptr
 * [B*L + 1]; cellmap [B][L][L] = cell id or -1.  The caller sizes cells from the count of listed cells. */
int smin_build_cells(void* stream, const uint8_t* mask, int B, int L, int all_cells,
                     int32_t* cells, int32_t* row_ptr, int32_t* cellmap);
/* The same for a caller that already knows the number of listed cells (a captured step replays with the count it was captured
 * for: no device -> host round trip inside the step).  cells holds exactly n_expected entries and nothing is written past it.
 * The caller gets the layout of the mask's first n_expected listed cells in (b, i, j) order: no row_ptr entry exceeds n_expected,
 * a listed cell past the cut has cellmap -1, and where the mask lists fewer cells, entries total .. n_expected - 1 of cells are
 * {0, 0, 0, 0} and belong to no row.  *status (device int32, cleared once by the caller) is set to 1 if the mask lists a
 * different number of cells, and is left as found otherwise. */
int smin_build_cells_n(void* stream, const uint8_t* mask, int B, int L, int all_cells, int n_expected,
                       int32_t* cells, int32_t* row_ptr, int32_t* cellmap, int32_t* status);

/* What the train step derives from its masks and the boundary heads' parameters before its first real kernel, in one launch
 * (main.py:141-160 hands the batch over as it comes from the dataset: byte masks): len32 [B] = words per query, qmf [B][Nq] /
 * vmaskf [B][T] / lmf [B][L] = the masks as fp32, *count (device int64) = number of set cells of moment_mask [B][L][L],
 * wb [3][D] / bb [3] = weights and biases of the start / end / "all" heads side by side (Localization, models.py:318-333; w, b:
 * HOST arrays of three device pointers).  Masks: one byte per element.  acc: 16 bytes of device memory, zero on entry and on exit. */
int smin_step_prologue(void* stream, const uint8_t* query_mask, const uint8_t* video_mask, const uint8_t* length_mask, const uint8_t* moment_mask,
                       const float* const* w, const float* const* b, int B, int Nq, int T, int L, int D, int32_t* len32, float* qmf, float* vmaskf,
                       float* lmf, float* wb, float* bb, int64_t* count, void* acc);

/* ---- layout helpers: dense (B,L,L,W) <-> packed [N][W] rows (W floats per cell). */
int smin_pack_cells(void* stream, const float* dense, const int32_t* cells, int N, int L, int W, float* packed);
int smin_unpack_cells(void* stream, const float* packed, const int32_t* cells, int N, int L, int W, float* dense /* pre-zeroed */);

/* ---- parameter-only operands of the content stream and the moment unit, every layer in one launch per direction
 * (csrc/param_prep.hip).  params: HOST array of nl*8 device pointers, per layer [Wch (dl,D) = linear_c_hat.weight, bch, Wc (D,dl) =
 * linear_c.weight, bc, Wfb (D,D) = conv_layer_fb.weight, bfb, Wfc (D,D) = conv_layer_fc.weight, bfc]  (models.py:247, 269, 288-303).
 *   Pcat: HOST array of nl*2 device pointers; entry [k*2 + part] (k > 4*part) is [dl][nseg*dl], nseg = min(4, k - 4 part), column block
 *         s = Wch_k Wc_{4 part + s};   consts [nl][dl] = bch_k + Wch_k (bc_0 + .. + bc_{k-1});   Wcat [nl][D][2D] = [Wfb_k | Wfc_k];
 *         bcat [nl][D] = bfb_k + bfc_k;   Wch_all [nl*dl][D].       nl <= 8, D % 32 == 0, D <= 1056, dl % 32 == 0.
 * Backward: dPcat (as Pcat), dconsts, dWcat, dbcat, dWch_all; *_base: HOST arrays of nl device pointers with the gradient a parameter
 * already has from its direct uses (dWch_base[k] may be NULL); grads: HOST array of nl*8 device pointers, every entry written. */
int smin_param_prep_fwd(void* stream, const float* const* params, int nl, int D, int dl, float* const* Pcat, float* consts, float* Wcat,
                        float* bcat, float* Wch_all);
int smin_param_prep_bwd(void* stream, const float* const* params, int nl, int D, int dl, const float* const* dPcat, const float* dconsts,
                        const float* dWcat, const float* dbcat, const float* dWch_all, const float* const* dWch_base,
                        const float* const* dWc_base, const float* const* dbc_base, float* const* grads);

/* ---- host helpers of the fused step: many small tensors in one launch.  src/dst/rows/cols/srcs are HOST arrays.
 *   smin_transpose_batch: dst[m] [cols][rows] = src[m]^T for n <= SMIN_BATCH_MAX row-major matrices src[m] [rows][cols]
 *     (the W^T operands of the input-gradient contractions; the reference transposes inside autograd, models.py every nn.Linear);
 *   smin_sum_lists: out[i] = sum_k srcs[k][i] in list order (gradients of f_s / f_w, which every layer consumes). */
#define SMIN_BATCH_MAX 32
int smin_transpose_batch(void* stream, const float* const* src, float* const* dst, const int32_t* rows, const int32_t* cols, int n);
int smin_sum_lists(void* stream, const float* const* srcs, int n, size_t numel, float* out);
/* out[c] = sum_r x[r][c]  (x [R][W], W % 4 == 0, W <= 1024): the bias gradient of a linear map whose weight gradient has no pass of its own
 * to ride on (content stream: layer 0's constant).  Two fixed-order stages. */
size_t smin_col_sum_workspace_bytes(int R, int W);
int smin_col_sum(void* stream, const float* x, int R, int W, float* out, void* ws, size_t ws_bytes);

/* ---- Adam / AdamW update of a parameter list with the gradients' global norm on the device (csrc/optimizer.hip).
 * param / grad / numel / moment_offset: HOST arrays of n entries (device pointers, element counts, first element of the tensor's segment
 * in the two flat fp32 moment buffers exp_avg / exp_avg_sq).  Tensors need no alignment: 16-byte loads and stores where param, grad and
 * both segments are 16-byte aligned, 4-byte ones otherwise and for a tensor's last numel % 4 elements.  grad is never written.
 *   state: 8 doubles on the device -- [0] t, completed steps; [1] beta1^t; [2] beta2^t (running products, one multiplication per
 *   step); [3] learning rate; [4] total gradient norm of the last step; [5] the clip coefficient it used (an fp32 value); [6] skipped
 *   steps; [7] non-finite flag of the last step.  The update reads the state; one closing wave behind it advances [0..2], or [6].
 * Per element, every fp32 operation rounded on its own, with B1 = state[1] * beta1, B2 = state[2] * beta2, step_size =
 * (float)(lr / (1 - B1)), sbc2 = (float)sqrt(1 - B2) formed in double and the constants rounded once to fp32:
 *   g = grad * c                       (only when the norm ran; c = state[5])
 *   g = g + wd * p                     (weight_decay != 0, decoupled == 0)          p = p - (float)(lr * wd) * p   (decoupled != 0)
 *   m = beta1 * m + (1 - beta1) * g    v = beta2 * v + ((1 - beta2) * g) * g        p = p - step_size * (m / (sqrtf(v) / sbc2 + eps))
 * Launches: ceil(non-empty tensors / 96) updates + 1 closing wave; none when n == 0 or every tensor is empty.
 * The norm entry, issued before the step on the same stream when clipping or the guard is wanted: per 4096-element chunk a partial sum of
 * (double)g * (double)g, the partials added in a fixed order by one workgroup (no atomics: the same bits every run); it writes
 * state[4] = sqrt(sum), state[5] = (float)min(1, max_norm / (norm + 1e-6)) -- 1 when max_norm < 0: guard only -- and state[7] = 1 when
 * the sum is inf or NaN.  ws: the partials, sized by the query below from the list's total element count.
 * The step entry with norm_ws != NULL scales by state[5]; with skip_nonfinite != 0 (which needs norm_ws) and state[7] set it writes
 * nothing and the closing wave adds 1 to state[6] instead of advancing t.  With norm_ws == NULL the closing wave sets [4] = NaN (not
 * formed), [5] = 1, [7] = 0.
 * Rejected before any launch: n < 0, a negative count or offset, a NULL pointer with a positive count, betas outside [0, 1), eps < 0,
 * weight_decay < 0, a NaN max_norm, a workspace that is too small. */
size_t smin_adam_ws_bytes(int64_t total_numel, int n);
int smin_grad_norm(void* stream, const float* const* grad, const int64_t* numel, int n, double max_norm, double* state, void* ws,
                   size_t ws_bytes);
int smin_adam_step(void* stream, float* const* param, const float* const* grad, const int64_t* numel, const int64_t* moment_offset, int n,
                   float* exp_avg, float* exp_avg_sq, double* state, double beta1, double beta2, double eps, double weight_decay,
                   int decoupled, int skip_nonfinite, const void* norm_ws);

/* ---- lazy Adam over the rows of a table listed by the rows entry of the token lookup's backward (csrc/row_sparse.hip).
 * table / exp_avg / exp_avg_sq [V][E] (16-byte aligned, E % 4 == 0); ids [n], rows [n][E], count [1], sqnorm [1] as that entry writes
 * them, or as smin_row_lists_merge does (n <= 65536 is the capacity of ids / rows; sqnorm may be NULL: norm unknown).  state: the 8 doubles of the step entry above, same
 * layout and rules; [4] = sqrt(sqnorm) (NaN without sqnorm), [5] = the scale used.  scale: NULL, or one double on the device (e.g.
 * state[5] of the model's optimizer), cast once to fp32.  One workgroup per slot s < count applies to row ids[s], every fp32 operation
 * rounded on its own and the scalars formed as above:
 *   g = rows[s] * (float)scale         (only when scale is given)
 *   m = beta1 * m + (1 - beta1) * g    v = beta2 * v + ((1 - beta2) * g) * g        p = p - step_size * (m / (sqrtf(v) / sbc2 + eps))
 * Rows not listed (and a slot whose id lies outside [0, V)) are neither read nor written; there is no weight decay.  One closing wave
 * advances t and the powers once per call, also when count == 0.  With skip_nonfinite != 0, an inf or NaN sqnorm or scale writes
 * nothing, leaves t alone and adds 1 to state[6]; state[7] is that flag either way.  Two launches (one when n == 0); no host read. */
int smin_row_adam_step(void* stream, float* table, float* exp_avg, float* exp_avg_sq, const int32_t* ids, const float* rows,
                       const int32_t* count, const double* sqnorm, int n, int V, int E, double* state, const double* scale, double beta1,
                       double beta2, double eps, int skip_nonfinite);

/* ---- merge of R row lists of one [V][E] table into one (csrc/row_sparse.hip): the gradients of data-parallel ranks
 * or of micro-batches.  ids / rows / count are HOST arrays of R device pointers, n a HOST array with the capacity of each list; scale is
 * NULL or one double on the device; the outputs have capacity N = the sum of n[r]; ws of the query below (8-byte aligned).
 * Inputs.  List r is as smin_embed_tokens_bwd_rows writes it: slots s < c_r hold strictly ascending ids in [0, V), with
 *   c_r = min(count_r[0], n[r]) clamped on the device.  rows_r[s] for s >= c_r is never read.  Limits: 1 <= R <= 16, n[r] >= 0,
 *   N <= 65536, E >= 4, E % 4 == 0, rows 16-byte aligned.  A list with n[r] == 0 is not read at all (its pointers may be NULL).
 * Ids.  out_ids[0 .. out_count) is the strictly ascending union of the listed ids; out_ids[out_count .. N) is -1; out_count[0] is the
 *   size of the union.
 * Rows.  out_rows[s] = ((rows_r0[.] + rows_r1[.]) + ...) over the lists that hold out_ids[s], in ascending r; every fp32 addition is
 *   rounded on its own.  When scale != NULL the row is then multiplied by (float)scale[0], cast once, with one more rounding.  Rows of
 *   slots >= out_count are not written.
 * Squared norm.  out_sqnorm[0] is the sum of squares of the out_count output rows in double, accumulated in the order of the rows entry
 *   above (per row: each thread over its quads in index order, then a fixed tree; then the rows in a fixed order).  With R = 1 and no
 *   scale the call therefore reproduces ids, rows, count and sqnorm of its input bit for bit.
 * Determinism.  The same bits every run (no atomics); four launches sized by N that exit early on device-side counts (N == 0: count
 *   and sqnorm are cleared, nothing is launched).  No host read.  No pass over V * E.
 * Malformed lists.  Every index formed from list contents is bounded before it is used: a list that breaks the ordering contract gives
 *   unspecified rows but no access outside the buffers.
 * Rejection.  A nonzero status is returned before any launch for: R outside [1, 16], a negative n[r], N > 65536, bad E, a NULL pointer
 *   with N > 0 (a list's own pointers only when n[r] > 0), misaligned rows, or a workspace that is too small. */
size_t smin_row_lists_merge_workspace_bytes(int R, int N);
int smin_row_lists_merge(void* stream, const int32_t* const* ids, const float* const* rows, const int32_t* const* count, const int* n,
                         int R, int V, int E, const double* scale, int32_t* out_ids, float* out_rows, int32_t* out_count,
                         double* out_sqnorm, void* ws, size_t ws_bytes);

/* ---- corpus search (csrc/corpus.hip): Q queries against a bank of V videos, each encoded once.
 * smin_pair_assemble has a backward, smin_pair_assemble_bwd below (training through shared banks); the two merges
 * (smin_corpus_topk, smin_search_merge) only rank and have none; smin_mine_pairs picks the pairs to train on.
 *
 * smin_pair_assemble: the backbone's outputs of P (video, query) pairs from the banks, one launch.
 * Inputs.  fv [V][T][D]: the video encoder's projection with position embedding and mask (smin_video_encoder_fwd with fs == NULL);
 *   fs_bank [Q][D], fw_bank [Q][Nq][D]: the query encoder's sentence and word features; video_index, query_index: [P] int32 on the
 *   device, any lists, repeats included.
 * Outputs.  f [P][T][D]: f[p][t][:] = fv[vi[p]][t][:] * fs_bank[qi[p]][:]; fw [P][Nq][D] = fw_bank[qi[p]]; fs [P][D] = fs_bank[qi[p]].
 * Arithmetic.  One fp32 multiplication per element of f, so its bits are those of smin_video_encoder_gate on expanded copies of the
 *   operands; the two gathers are bit copies.  16-byte loads and stores throughout.
 * Bounds.  An index outside [0, V) or [0, Q) is clamped into the range before it forms an address: the call cannot leave the buffers
 *   (the Python host refuses such an index before it gets here).
 * Limits.  D >= 4, D % 4 == 0, P, V, Q, T, Nq >= 1, buffers 16-byte aligned.  The outputs must not overlap the inputs.
 * Determinism.  The same bits every run (no atomics); no host read; capturable.
 * Rejection.  A nonzero status is returned before the launch for a bad D, a size below 1 or a NULL pointer. */
int smin_pair_assemble(void* stream, const float* fv, const float* fs_bank, const float* fw_bank, const int32_t* video_index,
                       const int32_t* query_index, int P, int V, int Q, int T, int Nq, int D, float* f, float* fw, float* fs);

/* smin_pair_assemble_bwd: the adjoint of smin_pair_assemble -- the gradients of the P pairs' f, f_w, f_s summed back onto the V videos
 * and Q queries they were gathered from.  Two launches, no atomics.
 * Inputs.  df [P][T][D], dfw [P][Nq][D], dfs [P][D]: the gradients of smin_pair_assemble's three outputs; dfw and dfs may each be NULL
 *   (= zeros, bit for bit).  fv [V][T][D], fs_bank [Q][D]: the forward's operands.  video_index, query_index: [P] int32 on the device,
 *   the forward's lists.  The same pairs grouped by video and by query, CSR, int32 on the device: v_ptr [V + 1] / v_pairs [P] -- video v
 *   owns v_pairs[v_ptr[v] .. v_ptr[v + 1]) --, q_ptr [Q + 1] / q_pairs [P]; each segment lists its pairs p in ascending order.  A
 *   segment names its video, so the kernels read fv[v] for the pairs of segment v and never read video_index (it is part of the
 *   signature as the list the segments were built from).
 * Outputs, every element written (nothing needs zeroing first).
 *   dfv [V][T][D]:       dfv[v][t][:]  = sum_{p in seg_v} df[p][t][:] * fs_bank[qi[p]][:]
 *   dfw_bank [Q][Nq][D]: dfw_bank[q]   = sum_{p in seg_q} dfw[p]
 *   dfs_bank [Q][D]:     dfs_bank[q][:] = sum_{p in seg_q} ( dfs[p][:] + sum_t df[p][t][:] * fv[vi[p]][t][:] )
 *   A video or a query with no pair gets exact zeros.
 * Order.  fp32; every sum starts at +0 and runs over the segment in list order.  dfv: one fused multiply-add per pair.  dfs_bank: a
 *   pair's dot over t is formed in chunks of 4 consecutive frames, each a chain of fused multiply-adds in ascending t from +0; chunk
 *   c belongs to lane c % 8; lane j adds, pair after pair in list order, its chunks in ascending c (lane 0 adds dfs[p] ahead of the
 *   pair's chunks); the eight lanes are then added in ascending j.  A function of the arguments only.
 * Traffic.  df is read once, fv once (not once per pair), fs_bank once per pair; the chunk dots pass through ws: P * ceil(T / 4) * D
 *   floats written and read.  16-byte loads and stores throughout.
 * Bounds.  Every value read from v_ptr, q_ptr (into [0, P], ascending), v_pairs, q_pairs (into [0, P)) and query_index (into [0, Q)) is
 *   clamped before it forms an address: malformed lists give unspecified sums, never an access outside the buffers.
 * Limits.  D >= 4, D % 4 == 0, P, V, Q, T, Nq >= 1, buffers 16-byte aligned; outputs and ws must not overlap the inputs or each other.
 * Workspace.  ws_bytes >= smin_pair_assemble_bwd_workspace_bytes(P, T, D), exactly P * ceil(T / 4) * D * 4.
 * Determinism.  The same bits every run; no host read; capturable.
 * Rejection.  A nonzero status before any launch for a bad D, a size below 1, a NULL pointer other than dfw / dfs, or a workspace that
 *   is too small; the outputs are then untouched. */
size_t smin_pair_assemble_bwd_workspace_bytes(int P, int T, int D);
int smin_pair_assemble_bwd(void* stream, const float* df, const float* dfw, const float* dfs, const float* fv, const float* fs_bank,
                           const int32_t* video_index, const int32_t* query_index, const int32_t* v_ptr, const int32_t* v_pairs,
                           const int32_t* q_ptr, const int32_t* q_pairs, int P, int V, int Q, int T, int Nq, int D, float* dfv,
                           float* dfw_bank, float* dfs_bank, void* ws, size_t ws_bytes);

/* smin_corpus_topk: the K best moments of each query over all of its videos, one launch, one workgroup per query; no workspace.
 * Inputs.  The per-pair lists exactly as smin_top_moments writes them for P pairs at k = k_video: pair_score [P][k_video] fp32,
 *   pair_idx [P][k_video][2] int64, pair_count [P] int32; pair_video [P] int32: each pair's video; pair_ptr [Q + 1] int32: query q owns
 *   pairs pair_ptr[q] .. pair_ptr[q + 1] (ascending, within [0, P]: P itself is not an argument and the range is trusted; a negative
 *   or descending entry gives an empty range).  A query may have no pairs, and the number of pairs per query is not limited.
 * Candidates.  The first min(pair_count[p], k_video) slots of each of the query's pairs, the count clamped on the device (a negative
 *   one lists nothing).  Slots past the count are never read.
 * Order.  Higher score first; ties go to the lower video index, then to the lower slot, then (two pairs of one query that name the
 *   same video) to the earlier pair.  A score of -0 counts as +0.  No suppression across videos: moments of different videos do not
 *   overlap, and within a video smin_top_moments has already applied the NMS.
 * Outputs.  The first K candidates in that order: out_video [Q][K] int64, out_idx [Q][K][2] int64 and out_score [Q][K] fp32 (idx and
 *   score copied bit for bit), out_count [Q] int32 = the number listed.  Empty slots: video -1, idx -1, score 0.
 * Limits.  1 <= K <= 64, 1 <= k_video <= 64, Q >= 0 (Q == 0: nothing is launched).
 * Determinism.  The same bits every run (no atomics); no host read; capturable.
 * Rejection.  A nonzero status is returned before the launch for a bad K or k_video, a negative Q, or, with Q > 0, a NULL pair_ptr or
 *   output.  Whether a query has pairs is known on the device only: with a NULL pair_score, pair_idx, pair_count or pair_video none of
 *   the four is read and every query comes out empty. */
int smin_corpus_topk(void* stream, const float* pair_score, const int64_t* pair_idx, const int32_t* pair_count, const int32_t* pair_video,
                     const int32_t* pair_ptr, int Q, int k_video, int K, int64_t* out_video, int64_t* out_idx, float* out_score,
                     int32_t* out_count);

/* smin_search_merge: S ranked lists per query, each over its own shard of the videos, into the K best of all shards; one launch, one
 * workgroup per query, no workspace, no host read; capturable.
 * Inputs.  video, idx, score, count: HOST tables of S device pointers, read before the call returns (they travel to the kernel by
 *   value); list s is smin_corpus_topk's output at K = k_list[s]: video [Q][k_s] int64, idx [Q][k_s][2] int64, score [Q][k_s] fp32,
 *   count [Q] int32.  k_list, video_offset: host [S]; video_offset[s] is added to list s's video ids (the shard's first global id).
 * Candidates.  Position p of list s for query q iff p < clamp(count_s[q], 0, k_s); what lies behind the counts is never read.
 * Order.  Higher score first (-0 counts as +0); ties go to the lower global video video_s[q][p] + video_offset[s], then to the lower
 *   s, then to the lower p.  EACH LIST IS ASSUMED ORDERED AS smin_corpus_topk ORDERS IT (not checked): then, for shards of disjoint
 *   videos given in ascending offset, the result is bit for bit smin_corpus_topk's list of the whole corpus, merged at once or folded
 *   one shard after another.  Global video ids must lie in [0, 2^31): the order key holds them as int32.
 * Outputs.  As smin_corpus_topk: out_video [Q][K] int64 global ids, out_idx [Q][K][2], out_score [Q][K] (idx and score copied bit for
 *   bit), out_count [Q]; empty slots -1 / -1 / 0.
 * Limits.  1 <= S <= 16, 1 <= K <= 64, 1 <= k_list[s] <= 64, 0 <= video_offset[s] < 2^31, Q >= 0 (Q == 0: returns 0, nothing launched).
 * Rejection.  A nonzero status before any launch for S, K or a k out of range, Q < 0, and with Q > 0 a NULL table, table entry or
 *   output, an offset out of range, or an output that is one of the input pointers. */
int smin_search_merge(void* stream, int S, const int64_t* const* video, const int64_t* const* idx, const float* const* score,
                      const int32_t* const* count, const int32_t* k_list, const int64_t* video_offset, int Q, int K,
                      int64_t* out_video, int64_t* out_idx, float* out_score, int32_t* out_count);

/* smin_corpus_span_topk: the K best span-valued moments of each query over all of its videos (SMIN.search_windows):
 * smin_corpus_topk for lists whose moments are spans in raw rows of long videos.  One launch, one workgroup per query; no workspace.
 * Inputs.  The per-group lists exactly as smin_merge_window_moments writes them for G2 (query, video) groups at k = k_video:
 *   span [G2][k_video][2] fp32, score [G2][k_video] fp32, window [G2][k_video] int64, cell [G2][k_video][2] int64, count [G2] int32;
 *   group_video [G2] int32: each group's video; group_ptr [Q + 1] int32: query q owns groups group_ptr[q] .. group_ptr[q + 1]
 *   (ascending, within [0, G2]: G2 itself is not an argument and the range is trusted; a negative or descending entry gives an empty
 *   range).  A query may have no groups, and the number of groups per query is not limited.
 * Candidates.  The first clamp(count[g], 0, k_video) slots of each of the query's groups, the count clamped on the device.  What lies
 *   behind the counts (NaN spans, -1) is never read.
 * Order.  smin_corpus_topk's, through the same order word: higher score first (-0 counts as +0); ties go to the lower video, then to
 *   the lower slot, then to the earlier group.  No suppression across videos; within a video smin_merge_window_moments has applied it.
 * Outputs.  The first K candidates in that order: out_video [Q][K] int64, out_span [Q][K][2] fp32, out_score [Q][K] fp32, out_window
 *   [Q][K] int64 and out_cell [Q][K][2] int64 (span, score, window and cell copied bit for bit), out_count [Q] int32 = the number
 *   listed.  Every element of every output is written; empty slots: video -1, span NaN (0x7fc00000), score 0, window -1, cell -1.
 * Limits.  1 <= K <= 64, 1 <= k_video <= 64, Q >= 0 (Q == 0: nothing is launched).  The outputs must not overlap the inputs.
 * Determinism.  The same bits every run (no atomics); no host read; capturable.
 * Rejection.  A nonzero status is returned before the launch for a bad K or k_video, a negative Q, or, with Q > 0, a NULL group_ptr or
 *   output.  Whether a query has groups is known on the device only: with a NULL span, score, window, cell, count or group_video none
 *   of the six is read and every query comes out empty. */
int smin_corpus_span_topk(void* stream, const float* span, const float* score, const int64_t* window, const int64_t* cell,
                          const int32_t* count, const int32_t* group_video, const int32_t* group_ptr, int Q, int k_video, int K,
                          int64_t* out_video, float* out_span, float* out_score, int64_t* out_window, int64_t* out_cell,
                          int32_t* out_count);

/* smin_span_search_merge: S ranked lists of span-valued moments per query, each over its own shard of a corpus of long videos, into
 * the K best of all shards: smin_search_merge for smin_corpus_span_topk's lists.  One launch, one workgroup per
 * query, no workspace, no copy, no atomics, no host read; capturable.
 * Inputs.  video, span, score, window, cell, count: HOST tables of S device pointers, read before the call returns (they travel to the
 *   kernel by value); list s is smin_corpus_span_topk's output at K = k_list[s]: video [Q][k_s] int64 (shard-local), span [Q][k_s][2]
 *   fp32, score [Q][k_s] fp32, window [Q][k_s] int64, cell [Q][k_s][2] int64, count [Q] int32.  k_list, video_offset: host [S];
 *   video_offset[s] is added to list s's video ids (the shard's first global id).
 * Candidates.  Position p of list s for query q iff p < clamp(count_s[q], 0, k_s); what lies behind the counts (NaN spans, -1) is
 *   never read.
 * Order.  smin_search_merge's: higher score first (-0 counts as +0); ties go to the lower global video video_s[q][p] +
 *   video_offset[s], then to the lower s, then to the lower p.  EACH LIST IS ASSUMED ORDERED AS smin_corpus_span_topk ORDERS IT (not
 *   checked): a candidate's rank is then p plus, over the other lists, the number of entries that go ahead of it (a binary search
 *   each: one pass, not K rounds), the ranks of a query are a permutation, and for shards of whole, disjoint videos given in
 *   ascending offset the result is bit for bit smin_corpus_span_topk's list of the whole corpus, merged at once or folded one shard
 *   after another.  For lists not so ordered the content is unspecified; every write stays in bounds and every element is written.
 *   Global video ids must lie in [0, 2^31): the order word holds them as int32.
 * Outputs.  As smin_corpus_span_topk: out_video [Q][K] int64 global ids, out_span [Q][K][2], out_score [Q][K], out_window [Q][K],
 *   out_cell [Q][K][2] (span, score, window and cell copied bit for bit), out_count [Q] = min(sum of the clamped counts, K).  Every
 *   element of every output is written; empty slots: video -1, span NaN (0x7fc00000), score 0, window -1, cell -1.
 * Limits.  1 <= S <= 16, 1 <= K <= 64, 1 <= k_list[s] <= 64, 0 <= video_offset[s] < 2^31, Q >= 0 (Q == 0: returns 0, nothing launched).
 * Determinism.  The same bits every run: each slot's last writer is fixed by the ranks.
 * Rejection.  A nonzero status before any launch for S, K or a k out of range, Q < 0, and with Q > 0 a NULL table, table entry or
 *   output, an offset out of range, or an output that is one of the input pointers. */
int smin_span_search_merge(void* stream, int S, const int64_t* const* video, const float* const* span, const float* const* score,
                           const int64_t* const* window, const int64_t* const* cell, const int32_t* const* count,
                           const int32_t* k_list, const int64_t* video_offset, int Q, int K, int64_t* out_video, float* out_span,
                           float* out_score, int64_t* out_window, int64_t* out_cell, int32_t* out_count);

/* smin_search_merge_weighted, smin_span_search_merge_weighted: S shard lists that carry their UNWEIGHTED moment scores, merged into
 * the K best per query under the video weights and ranks of all the shards' videos.  One launch, one workgroup of
 * 256 per query, 8 KB of LDS, no workspace, no atomics, no host read; capturable.  The two differ in what an entry holds beside video,
 * raw and score: idx [.][2] int64 (smin_corpus_topk's lists) or span [.][2] fp32, window int64 and cell [.][2] int64
 * (smin_corpus_span_topk's); one templated kernel body.
 * Inputs.  video, idx (span, window, cell), raw, count: HOST tables of S device pointers, read before the call returns; list s holds
 *   video [Q][k_s] int64 (local to the list), the entry fields, raw [Q][k_s] fp32 -- the entry's moment score before any video weight --
 *   and count [Q] int32.  k_list, video_offset: host [S]; video_offset[s] is added to list s's video ids.  video_rank [Q][V] int32
 *   (-1: not a candidate video) and video_weight [Q][V] fp32 on the device: smin_video_rank's pair_rank and weight over the V global
 *   videos (pair_ptr[q] = q * V, pair_video = v).  max_videos <= 0: no cut.
 * Candidates.  Position p of list s for query q iff p < clamp(count_s[q], 0, k_s); with g = video_s[q][p] + video_offset[s] it drops
 *   out unless 0 <= g < V (g forms no address before that check), video_rank[q][g] >= 0 and (max_videos <= 0 or video_rank[q][g] <
 *   max_videos).  Its value is raw * video_weight[q][g], one fp32 multiplication: smin_moment_reweight's expression, the same bits.
 * Order.  Higher value first (-0 counts as +0); ties go to the lower g, then to the lower s, then to the lower p.  THE LISTS ARE NOT
 *   ASSUMED SORTED in that order (they were ranked under other weights, and rounding may swap near-ties): the surviving candidates'
 *   order words are staged in LDS and each counts the words ahead of it, as smin_video_rank does -- a strict total order, so the ranks
 *   are a permutation and, after the fill with the empty pattern, every slot below out_count has exactly one writer.
 * Outputs, every element written.  out_video [Q][K] int64 = g; the entry fields and out_raw [Q][K] moved bit for bit; out_score [Q][K]
 *   the value; out_count [Q] = min(survivors, K).  Empty slots: video -1, idx / window / cell -1, span NaN (0x7fc00000), score and
 *   raw 0.  The result is a list of the same form over global ids: a later merge takes it at offset 0.
 * Limits.  1 <= S <= 16, 1 <= K <= 64, 1 <= k_list[s] <= 64, 0 <= video_offset[s] < 2^31, V >= 0 (V == 0: the two video tables may be
 *   NULL, every query comes out empty), Q >= 0 (Q == 0: returns 0, nothing launched).
 * Determinism.  The same bits every run: ranks are counts, each slot's last writer is fixed by them.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for S, K or a k out of range, Q < 0, V < 0, and with Q > 0 a
 *   NULL table, table entry or output, an offset out of range, or an output that is one of the input pointers. */
int smin_search_merge_weighted(void* stream, int S, const int64_t* const* video, const int64_t* const* idx, const float* const* raw,
                               const int32_t* const* count, const int32_t* k_list, const int64_t* video_offset, const int32_t* video_rank,
                               const float* video_weight, int V, int max_videos, int Q, int K, int64_t* out_video, int64_t* out_idx,
                               float* out_score, float* out_raw, int32_t* out_count);
int smin_span_search_merge_weighted(void* stream, int S, const int64_t* const* video, const float* const* span, const float* const* raw,
                                    const int64_t* const* window, const int64_t* const* cell, const int32_t* const* count,
                                    const int32_t* k_list, const int64_t* video_offset, const int32_t* video_rank, const float* video_weight,
                                    int V, int max_videos, int Q, int K, int64_t* out_video, float* out_span, float* out_score,
                                    float* out_raw, int64_t* out_window, int64_t* out_cell, int32_t* out_count);

/* smin_mine_pairs: the pair plan of hard-negative mining -- for each of Q queries its own video and the N
 * highest-scoring wrong videos, as smin_pair_assemble's two lists and smin_pair_assemble_bwd's two groupings, formed on the device.
 * Four launches (select, count, scan, fill), no atomics.  P = Q * (1 + N); pair p = q * (1 + N) + s is slot s of query q.
 * Inputs.  score [Q][V] fp32: each (query, video) pair's score, expected finite (SMIN.pair_scores: the best fused moment score);
 *   gt_video [Q] int32 on the device: each query's own video, clamped into [0, V) before it forms an address or a comparison.
 *   skip: the number of hardest negatives left out (in moment retrieval those are often unlabelled true matches).
 * Order.  Among the videos v != gt_video[q]: higher score[q][v] first, ties go to the lower v, a score of -0 counts as +0 -- the
 *   order of smin_corpus_topk, found by the same rounds (one workgroup per query, skip + N block argmaxes of order keys).  With a
 *   NaN in the row the order is unspecified; the picks stay distinct, within [0, V) and != gt_video[q].
 * Outputs, all int32, every element written.
 *   query_index [P]:  query_index[p] = q.
 *   video_index [P]:  slot 0 = gt_video[q] (the positive pair); slots 1 .. N = the negatives of ranks skip .. skip + N - 1, in rank
 *     order.  A query's 1 + N videos are distinct.
 *   q_ptr [Q + 1], q_pairs [P]: the pairs grouped by query: q_ptr[q] = q * (1 + N), q_pairs[p] = p.
 *   v_ptr [V + 1], v_pairs [P]: the pairs grouped by video, each segment in ascending p; a segment holds at most Q pairs, a video no
 *     query picked an empty one.  Exactly the arrays a stable sort of video_index gives (bincount, cumsum, argsort).
 * Limits.  Q >= 1, V >= 2, N >= 1, skip >= 0, skip + N <= 64, skip + N <= V - 1, Q * (1 + N) < 2^31.  The outputs and ws must not
 *   overlap the inputs or each other.
 * Workspace.  ws_bytes >= smin_mine_pairs_ws_bytes(Q, V, N), exactly V * 4 (the videos' pair counts between the launches); the
 *   query returns 0 for Q < 1, V < 2 or N < 1.
 * Determinism.  The same bits every run: the outputs are a function of score and gt_video alone, placed with plain stores in a
 *   fixed order (no atomics, no library sort); no host read; capturable.
 * Rejection.  A nonzero status is returned before any launch, the outputs untouched, for a limit broken, a NULL pointer, or a
 *   workspace that is too small. */
size_t smin_mine_pairs_ws_bytes(int Q, int V, int N);
int smin_mine_pairs(void* stream, const float* score, const int32_t* gt_video, int Q, int V, int N, int skip, int32_t* video_index,
                    int32_t* query_index, int32_t* v_ptr, int32_t* v_pairs, int32_t* q_ptr, int32_t* q_pairs, void* ws, size_t ws_bytes);

/* ---- video-level contrastive loss over a pair plan (csrc/pair_rank.hip): each query's own video ranked above the
 * wrong ones it was paired with.  All arithmetic fp32.
 *
 * smin_pair_rank_fwd: three launches (pool, queries, total), no atomics.
 * Inputs.  pm [P][L][L], ps [P][L], pe [P][L] fp32: the P pairs' scores (forward_pairs); mm [P][L][L] one byte per cell: the pairs'
 *   moment_mask (nonzero = valid).  q_ptr [Q + 1], q_pairs [P] int32: the pairs grouped by query, CSR, query q owns
 *   q_pairs[q_ptr[q] .. q_ptr[q + 1]), in list order (a PairPlan's).  positive [P] int32: nonzero where the pair's video is its query's
 *   own.  tau: the temperature that pools a pair's cells, gamma: the one across a query's videos.
 * Cell score.  f[p][i][j] = (pm[p][i][j] * sqrtf(max(ps[p][i], 1e-12f))) * sqrtf(max(pe[p][j], 1e-12f)), smin_top_moments' order.
 * Pair score.  Over the pair's n_p valid cells, m_p their maximum: s_p = m_p + tau * logf((sum_valid expf((f - m_p) / tau)) / n_p);
 *   n_p == 0: s_p = 0, a constant that still takes part in its query's sums.
 * Query loss.  S_q the query's segment, S_q+ its pairs with positive != 0, M_q = max_{S_q} s, M_q+ = max_{S_q+} s:
 *   l_q = log sum_{S_q} exp(s_p / gamma) - log sum_{S_q+} exp(s_p / gamma), each sum shifted by the maximum of its own terms:
 *   l_q = (M_q - M_q+) / gamma + logf(sum_{S_q} expf((s_p - M_q) / gamma)) - logf(sum_{S_q+} expf((s_p - M_q+) / gamma)).
 *   Both sums are >= 1, so l_q and coef are finite however far a positive lies below the best negative, at any gamma for which
 *   (M_q - M_q+) / gamma is finite in fp32.
 *   A query with S_q+ empty (a query without a pair among them) is not counted.
 * Outputs, every element written.
 *   loss [1] = (sum of l_q over the Nc counted queries) / Nc, exactly 0 when Nc == 0.
 *   stats [2] = { Nc, hits }: a counted query is a hit when max_{S_q+} s >= max_{S_q \ S_q+} s (always, without a negative).
 *   pair_score [P] = s_p.
 *   coef [P]: (softmax_{S_q}(p) - [p in S_q+] softmax_{S_q+}(p)) / gamma, the derivative of l_q by s_p, 0 for the pairs of a query that
 *     is not counted (and for a pair no segment lists);  pool [P][2] = { m_p, the sum over the valid cells } (0, 0 when n_p == 0).
 *     stats, coef and pool are what smin_pair_rank_bwd reads.
 * Order.  Pool: one workgroup of 256 per pair; thread t takes cells t, t + 256, ... of the row-major map in ascending order, the 64
 *   lanes of a wave are added by wave_sum (DPP), the four waves as (w0 + w1) + (w2 + w3); the maximum first, then the sum.  Queries:
 *   one wave64 per query; lane l takes entries l, l + 64, ... of the segment in ascending order, then wave_sum.  Total: one thread
 *   adds l_q, the counted flags and the hits in ascending q.
 * Bounds.  Every value read from q_ptr (into [0, P], ascending) and q_pairs (into [0, P)) is clamped before it forms an address:
 *   malformed lists give unspecified sums, never an access outside the buffers.
 * Limits.  P, Q >= 1, 1 <= L <= 4096 (cells are counted in fp32), tau and gamma finite and > 0; ws 16-byte aligned; the outputs and
 *   ws must not overlap the inputs or each other.
 * Workspace.  ws_bytes >= smin_pair_rank_ws_bytes(P, Q, L), exactly Q * 16 (l_q and the two flags between the launches); the
 *   query returns 0 for a size out of range.
 * Determinism.  The same bits every run; no host read; no allocation; capturable.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for a size out of range, a NULL pointer, a tau or gamma that
 *   is not finite and positive, or a workspace that is too small. */
size_t smin_pair_rank_ws_bytes(int P, int Q, int L);
int smin_pair_rank_fwd(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const int32_t* q_ptr,
                       const int32_t* q_pairs, const int32_t* positive, int P, int Q, int L, float tau, float gamma, float* loss,
                       float* stats, float* pair_score, float* coef, float* pool, void* ws, size_t ws_bytes);

/* smin_pair_rank_bwd: the gradients of smin_pair_rank_fwd's loss by pm, ps and pe; one launch, one workgroup of 256 per pair, no
 * atomics, no workspace.  f and the exponentials are recomputed from the inputs, not stored.
 * Inputs.  dloss [1]: the upstream gradient; stats, coef, pool: the forward's; pm, ps, pe, mm, tau: the forward's.
 * Outputs, every element written.  With g_p = dloss * coef[p] / Nc and df = g_p * expf((f - m_p) / tau) / pool[p][1] on the valid cells,
 *   a_i = sqrtf(max(ps[p][i], 1e-12f)), b_j likewise of pe, and a', b' their derivatives with torch.clamp_min's gradient (0.5 / a where
 *   ps >= 1e-12f, else 0):
 *   dpm [P][L][L] = (df * a_i) * b_j, 0 in a masked cell;
 *   dps [P][L]    = (sum_j (df * pm) * b_j) * a'_i;    dpe [P][L] = (sum_i (df * pm) * a_i) * b'_j;  0 for a row or column without a
 *   valid cell.  A pair with g_p == 0 (its query not counted, Nc == 0) or without a valid cell gets zeros throughout.
 * Order.  dps: wave w takes rows w, w + 4, ...; lane l adds the columns l, l + 64, ... in ascending order, then wave_sum.  dpe: columns
 *   in chunks of 64, lane l has column chunk + l; wave w adds rows w, w + 4, ... in ascending order, and the four waves are added as
 *   (w0 + w1) + (w2 + w3).  A function of the arguments only.
 * Limits.  P >= 1, 1 <= L <= 4096, tau finite and > 0.  The outputs must not overlap the inputs or each other.
 * Determinism.  The same bits every run; no host read; no allocation; capturable.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range, a NULL pointer or a bad tau. */
int smin_pair_rank_bwd(void* stream, const float* dloss, const float* stats, const float* coef, const float* pool, const float* pm,
                       const float* ps, const float* pe, const uint8_t* mm, int P, int L, float tau, float* dpm, float* dps, float* dpe);

/* ---- listwise soft-target loss over a pair plan (csrc/pair_rank.hip): each query's softmax over its pair scores
 * pulled towards the softmax over a teacher's scores of the same pairs.  All arithmetic fp32.
 *
 * smin_pair_distill_fwd: three launches (pool, queries, total), no atomics; the first and the third are smin_pair_rank_fwd's kernels.
 * Inputs.  pm, ps, pe, mm, q_ptr, q_pairs, tau: as smin_pair_rank_fwd (no positive flags are read).  teacher [P] fp32: one score per
 *   pair, in pair order; it receives no gradient.  gamma: the temperature across a query's videos on the student's side,
 *   gamma_teacher: on the teacher's.
 * Pair score.  s_p of smin_pair_rank_fwd, BIT FOR BIT (the same kernel); n_p == 0: s_p = 0, and the pair still takes part.
 * Query loss.  S_q the query's segment, t_p = teacher[p]:
 *   xS_p = (s_p - max_{S_q} s) / gamma,          ZS = sum_{S_q} expf(xS),  pS_p = expf(xS_p) / ZS,  lS_p = xS_p - logf(ZS);
 *   xT_p = (t_p - max_{S_q} t) / gamma_teacher,  ZT, pT_p, lT_p likewise;
 *   l_q = sum_{S_q} pT_p * (lT_p - lS_p) = KL(teacher || student); no logf takes a probability.
 *   Both sides run one device function in one expression order: teacher == pair_score with gamma_teacher == gamma gives a loss and
 *   coefficients of exactly 0.
 *   A query is counted when its segment lists at least two pairs and every teacher value in it is finite.
 * Outputs, every element written.
 *   loss [1] = (sum of l_q over the Nc counted queries) / Nc, exactly 0 when Nc == 0.
 *   stats [2] = { Nc, agree }: a counted query agrees when the first entry in list order with the highest teacher score is also the
 *     first entry in list order with the highest pair score.
 *   pair_score [P] = s_p.
 *   coef [P]: (pS_p - pT_p) / gamma, the derivative of l_q by s_p, 0 for the pairs of a query that is not counted (and for a pair no
 *     segment lists);  pool [P][2]: as smin_pair_rank_fwd.
 * Backward.  smin_pair_rank_bwd as it stands, called with this forward's stats, coef and pool.
 * Order.  Pool and total: smin_pair_rank_fwd's.  Queries: one wave64 per query, four queries per workgroup; lane l takes entries l,
 *   l + 64, ... of the segment in ascending order; every total is wave_sum or wave_max of the lanes' partials.
 * Bounds.  Every value read from q_ptr (into [0, P], ascending) and q_pairs (into [0, P)) is clamped before it forms an address.
 * Limits.  P, Q >= 1, 1 <= L <= 4096, tau, gamma and gamma_teacher finite and > 0; ws 16-byte aligned; the outputs and ws must not
 *   overlap the inputs or each other.
 * Workspace.  ws_bytes >= smin_pair_distill_ws_bytes(P, Q, L), exactly Q * 16; the query returns 0 for a size out of range.
 * Determinism.  The same bits every run; no host read; no allocation; capturable.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for a size out of range, a NULL pointer, a tau, gamma or
 *   gamma_teacher that is not finite and positive, or a workspace that is too small. */
size_t smin_pair_distill_ws_bytes(int P, int Q, int L);
int smin_pair_distill_fwd(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const int32_t* q_ptr,
                          const int32_t* q_pairs, const float* teacher, int P, int Q, int L, float tau, float gamma, float gamma_teacher,
                          float* loss, float* stats, float* pair_score, float* coef, float* pool, void* ws, size_t ws_bytes);

/* ---- video ranking by the pooled pair score (csrc/video_rank.hip): the score smin_pair_rank_fwd contrasts, read
 * at inference.  All arithmetic fp32; no atomics, plain stores; no workspace; no host read; no allocation; capturable.
 *
 * smin_pair_pool: the pooled score of each of P maps; one launch, one workgroup of 256 per map.
 * Inputs.  pm [P][L][L], ps [P][L], pe [P][L] fp32, mm [P][L][L] one byte per cell (nonzero = valid), tau: as smin_pair_rank_fwd.
 * Outputs, every element written.  score [P] = s_p of smin_pair_rank_fwd, BIT FOR BIT its pair_score on the same inputs: both entry
 *   points run one copy of the device code (csrc/pair_pool.h), in smin_pair_rank_fwd's order -- thread t takes cells t, t + 256, ...,
 *   wave_sum, the four waves as (w0 + w1) + (w2 + w3), the maximum first and the sum second.  pool [P][2] = { m_p, sum_valid expf((f -
 *   m_p) / tau) }; cells [P] = n_p, the number of valid cells, as fp32 (exact: L <= 4096).  A pair without a valid cell: score 0, pool
 *   { 0, 0 }, cells 0.
 * Limits.  P >= 1, 1 <= L <= 4096, tau finite and > 0.  The outputs must not overlap the inputs or each other.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range, a NULL pointer or a bad tau. */
int smin_pair_pool(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int P, int L, float tau,
                   float* score, float* pool, float* cells);

/* smin_group_pool: the score of each (query, video) group of a window search -- the log-mean-exp over all valid cells of the group's
 * windows, composed from the windows' pools; one launch, one thread per group.
 * Inputs.  pool [W][2], cells [W] fp32: smin_pair_pool's outputs for the W (query, window) maps; group_ptr [G2 + 1] int32: group g owns
 *   windows group_ptr[g] .. group_ptr[g + 1]; every entry is clamped into [0, W] and made ascending before it forms an address.
 * Score.  Over the group's windows with cells[w] > 0, in ascending w: M = max m_w, then S = sum of sum_w * expf((m_w - M) / tau) and
 *   N = sum of cells_w; score [G2] = M + tau * logf(S / N), out_cells [G2] = N.  A group without windows or without cells: score 0,
 *   cells 0.  A CELL IN THE OVERLAP OF TWO WINDOWS COUNTS TWICE: the windows are pooled as they were scored, each over its own map.
 *   The order of every sum depends on the arguments only.
 * Limits.  G2 >= 0 (G2 == 0: nothing is launched), W >= 0 (W == 0: pool and cells may be NULL, every group comes out empty), tau
 *   finite and > 0.  Every element of both outputs is written.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a negative size, a bad tau or, with G2 > 0, a NULL
 *   pointer. */
int smin_group_pool(void* stream, const float* pool, const float* cells, const int32_t* group_ptr, int G2, int W, float tau, float* score,
                    float* out_cells);

/* smin_video_rank: per query, its videos ranked by the pair score; one launch, one workgroup of 256 per query.
 * Inputs.  pair_score [P], pair_cells [P] fp32: smin_pair_pool's (or smin_group_pool's) score and cell count of P (query, video) pairs;
 *   pair_video [P] int32: each pair's video; pair_ptr [Q + 1] int32: query q owns pairs pair_ptr[q] .. pair_ptr[q + 1], every entry
 *   clamped into [0, P] and made ascending before it forms an address; the number of pairs per query is not limited.  gt_video [Q]
 *   int32 or NULL: each query's own video (compared, never an index).  alpha: the weight's exponent scale.
 * Candidates.  The query's pairs with pair_cells > 0.
 * Order.  Higher score first (-0 counts as +0); ties go to the lower video, then to the earlier pair: smin_corpus_topk's order word.
 *   A pair's rank is the number of the query's candidates ahead of it, found by counting against the segment's order words, which go
 *   through LDS 2048 at a time: no sort, no rounds, any number of pairs.
 * Outputs, every element written (pair_rank and weight: for an ascending pair_ptr; the pairs in front of the first segment and behind
 *   the last are written as non-candidates).  A pair_ptr that is not ascending is clamped, so every access stays inside the buffers,
 *   but the clamped segments may then overlap -- a pair_rank / weight element gets two writers and holds either query's value --
 *   or leave pairs between them unwritten: the content is unspecified there, and the same bits every run are no longer promised.
 *   pair_rank [P] int32: the 0-based rank among the query's candidates, -1 for a non-candidate; not limited by n.
 *   weight [P]: expf(alpha * (s_p - s_max(q))) for a candidate, s_max the query's best candidate score; exactly 1.0f for every
 *     candidate when alpha == 0; 0 for a non-candidate.  alpha > 0 gives weights in (0, 1], alpha < 0 weights >= 1 (inf once
 *     alpha * (s_p - s_max) passes fp32's range: the caller's choice).
 *   out_video [Q][n] int64, out_score [Q][n] fp32 (copied bit for bit), out_count [Q] int32: the first min(n, candidates) candidates;
 *     empty slots: video -1, score 0.
 *   gt_rank [Q] int32: the rank of the candidate whose video is gt_video[q] (the best of them, should two pairs name it); -1 if no
 *     candidate of the query names it or gt_video is NULL.
 * Limits.  0 <= P <= 0x7fff0000 (P == 0: the four lists and pair_rank / weight may be NULL), Q >= 0 (Q == 0: nothing is launched),
 *   1 <= n <= 64, alpha finite, of either sign.  The outputs must not overlap the inputs or each other.
 * Determinism.  The same bits every run: ranks are counts, each output slot has one writer.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range, an alpha that is not finite or,
 *   with Q > 0, a NULL pointer other than gt_video. */
int smin_video_rank(void* stream, const float* pair_score, const float* pair_cells, const int32_t* pair_video, const int32_t* pair_ptr,
                    const int32_t* gt_video, int P, int Q, int n, float alpha, int64_t* out_video, float* out_score, int32_t* out_count,
                    int32_t* pair_rank, float* weight, int32_t* gt_rank);

/* smin_moment_reweight: the pairs' moment lists weighted by their video and cut to the best videos; one launch, one thread per slot.
 * Inputs.  score [P][k] fp32, count [P] int32: smin_top_moments' (or smin_merge_window_moments') lists of the P pairs; pair_rank [P],
 *   weight [P]: smin_video_rank's.
 * Outputs, every element written.  out_score [P][k] = score * weight[p], one fp32 multiplication (slots behind the count included:
 *   nothing reads them); out_count [P] = count[p] where max_videos <= 0 (no cut) or 0 <= pair_rank[p] < max_videos, else 0.  The lists
 *   keep their order (weight >= 0), so smin_corpus_topk and smin_corpus_span_topk rank them unchanged.
 * Limits.  P >= 0 (P == 0: nothing is launched), 1 <= k <= 64, P * k < 2^39.  The outputs must not overlap the inputs.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range or, with P > 0, a NULL pointer. */
int smin_moment_reweight(void* stream, const float* score, const int32_t* count, const int32_t* pair_rank, const float* weight, int P, int k,
                         int max_videos, float* out_score, int32_t* out_count);

/* ---- first-stage video score from the banks alone (csrc/prefilter.hip): the model with zero SMI layers -- the score
 * heads on ProposalGeneration's output --, which is linear in the video bank.  No atomics, plain stores; no host read; no allocation;
 * capturable.
 *
 * smin_prefilter_scores: the first-stage score of every (query, video) of Q queries and V videos; three launches.
 * Inputs.  fv [V][T][D] fp32: the video bank; fs [Q][D] fp32: the queries' sentence features; w [3][D], b [3] fp32: the weights and
 *   biases of the heads in the order (pm, ps, pe); lmask [V][L], mm [V][L][L]: one byte per entry (nonzero = valid), as the banks
 *   hold them; tau: the pooling temperature.
 * Stage 1.  a_h[q][v][t] = sum_d fv[v][t][d] * (fs[q][d] * w[h][d]): a small kernel forms the operand fs (.) w_h as [3 Q rounded up to
 *   4][D] rows (row 3 q + h; the padding rows are zero) and ONE contraction [V T][D] x [.][D]^T runs on the fp32 MFMA engine in the
 *   mode of smin_set_gemm_mode; its epilogue stores the projections transposed ([3 q + h][V T]) into the workspace.
 * Stage 2.  One workgroup of 256 per (q, v) stages the pair's 3 T projections in LDS.  With r = T / L:
 *   pm0[i][j] = sigmoid((S * (1.0f / (float)cs)) / (float)C + b[0]) where mm[v][i][j] != 0, else 0;  S = the sum of a_0[t] over t in
 *     [i r, i r + c cs), n = (j - i + 1) r, cs = max(1, n / C), c = min(C, n) (an empty range under the diagonal): the mean over C of
 *     the content matrix's clips, with 1 / cs rounded to fp32 as the reference stores it (csrc/proposal_map.hip does the same).  Lane i of wave 0 owns row i and keeps ONE running sum from frame i r on, frames in ascending order (the
 *     ranges of a row share their start and their ends do not decrease with j): at most T additions per row.
 *   ps0[i] = sigmoid(S_i / (float)r + b[1]) where lmask[v][i] != 0, else 0;  S_i = a_1[i r] + ... + a_1[i r + r - 1], ascending;  pe0
 *     likewise of a_2 and b[2].  sigmoid(x) = 1 / (1 + expf(-x)).
 *   score, pool, cells: smin_pair_pool's of (pm0, ps0, pe0, mm[v]) -- csrc/pair_pool.h, the one copy of that device code, so the bits
 *     are smin_pair_pool's on the stored maps.  A pair without a valid cell: score 0, pool { 0, 0 }, cells 0.
 * Outputs, every element written, pair p = q V + v:  score [Q][V], pool [Q][V][2], cells [Q][V] fp32;  pm0 [Q V][L][L], ps0 [Q V][L],
 *   pe0 [Q V][L] fp32: given together or all NULL (the scores do not depend on it).
 * Every (q, v) is computed alone: a call on a slice of the videos gives the slice's bits.
 * Workspace.  ws_bytes >= smin_prefilter_ws_bytes(Q, V, T, D) (0 for sizes out of range): the operand and the projections.
 * Limits.  1 <= Q <= 65535, V >= 1, 1 <= L <= 64, L <= T <= 2048, 1 <= C <= 65536, D >= 4 with D % 4 == 0, V T <= 0x7fff0000 and
 *   V T (3 Q + 3) <= 2^34 (call it on slices of the videos beyond that).  LDS per
 *   workgroup: 4 (3 T + L L + 4 L + 4) bytes.  The outputs and the workspace must not overlap the inputs or each other.
 * Determinism.  The same bits every run.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for a size out of range, D % 4 != 0, T < L, a bad tau, a NULL
 *   pointer (the three maps: only some of them NULL) or a short workspace. */
size_t smin_prefilter_ws_bytes(int Q, int V, int T, int D);
int smin_prefilter_scores(void* stream, const float* fv, const float* fs, const float* w, const float* b, const uint8_t* lmask,
                          const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float tau, float* score, float* pool, float* cells,
                          float* pm0, float* ps0, float* pe0, void* ws, size_t ws_bytes);

/* smin_prefilter_maps_bwd: the gradients of smin_prefilter_scores' maps by the banks and the heads: from dpm0,
 * dps0, dpe0 to dfv, dfs, dw and db.  Seven launches, the slab reduction among them; no atomics, plain stores; no host read; no allocation;
 * capturable.
 * Inputs.  dpm0 [Q V][L][L], dps0, dpe0 [Q V][L] fp32: the gradients on the maps, pair p = q V + v; pm0, ps0, pe0: the forward's stored
 *   outputs (the sigmoids' slopes y (1 - y) are taken from them); fv, fs, w, lmask, mm, Q, V, T, L, C, D: as smin_prefilter_scores.
 * Per pair, one workgroup of 256, with r = T / L, n = (j - i + 1) r, cs = max(1, n / C), c = min(C, n):
 *   g_m[i][j] = dpm0 pm0 (1 - pm0) where mm[v][i][j] != 0, else 0;  g_s[i] = dps0 ps0 (1 - ps0) where lmask[v][i] != 0, else 0;  g_e
 *     likewise.  (A masked entry's gradient is never used: it may hold anything.)
 *   dS[i][j] = (g_m[i][j] * (1.0f / (float)cs)) / (float)C for j >= i (1 / cs rounded to fp32 as the forward rounds it), else 0;
 *   da_m[t] = the sum of dS[i][j] over the cells whose range [i r, i r + c cs) holds frame t: four threads share a row of the map, a
 *     quarter each, and form the row's suffix sums (the ranges of a row share their start and their ends do not decrease with j), a
 *     table per (T, L, C) names the first j - i whose range reaches a given offset, and a frame adds ONE suffix sum per row, rows i
 *     ascending: L T lookups per pair;  da_s[t] = g_s[t / r] / (float)r, da_e likewise;  frames t >= L r: exactly 0.
 *   The pair's sums of g_m, g_s, g_e go to the workspace in fp64 -- under a contrastive loss the slopes cancel over a query's videos,
 *     some 300-fold on the tiny test model, and an fp32 running sum would spend its rounding on the partial sums --; a small kernel
 *     adds them into db over p ascending (lane k of 64 takes p = k, k + 64, ...; then the lanes ascending) and rounds once.
 * With da [V T][N3] (column 3 q + h; N3 = 3 Q rounded up to 4, the padding columns zero) and op[3 q + h] = fs[q] (.) w[h]:
 *   dfv = da op (the NT engine against op stored transposed, K = N3);  dop = da^T fv (the TN engine over the V T rows in sp row
 *   splits, the slabs added in split order);  dfs[q] = sum_h dop[3 q + h] (.) w[h], h ascending;  dw[h] = sum_q dop[3 q + h] (.) fs[q],
 *   q ascending.  Both contractions run in the mode of smin_set_gemm_mode.
 * Outputs, every element written.  dfv [V][T][D], dfs [Q][D], dw [3][D], db [3] fp32.
 * Workspace.  ws_bytes >= smin_prefilter_bwd_ws_bytes(Q, V, T, D) (0 for sizes out of range) = 4 (V T N3 + D N3 + sp N3 D + N3 D + 8 Q V)
 *   bytes, in that order: da, op transposed, the slabs, dop and the pairs' partial sums of db ([Q V][4] fp64); ws 16-byte aligned;
 *   sp = max(1, min(ceil(768 / (ceil(N3 / 128) ceil(D / 128))), ceil(V T / 64))).
 * Limits.  smin_prefilter_scores' (1 <= L <= 64, L <= T <= 2048, D % 4 == 0, ...) and (3 Q + 3) D <= 2^28.  LDS per workgroup:
 *   4 (L (L | 1) + 4 L + T + 24) bytes, under 26 KB at the limits.  The outputs and the workspace must not overlap the inputs or each
 *   other.
 * Determinism.  Every sum runs in an order fixed by the arguments: the same bits every run.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for a size out of range, a NULL pointer, a short or misaligned workspace or
 *   an output (the workspace included) that is one of the inputs or another output. */
size_t smin_prefilter_bwd_ws_bytes(int Q, int V, int T, int D);
int smin_prefilter_maps_bwd(void* stream, const float* dpm0, const float* dps0, const float* dpe0, const float* pm0, const float* ps0,
                            const float* pe0, const float* fv, const float* fs, const float* w, const uint8_t* lmask, const uint8_t* mm,
                            int Q, int V, int T, int L, int C, int D, float* dfv, float* dfs, float* dw, float* db, void* ws,
                            size_t ws_bytes);

/* smin_prefilter_select: each query's best Ms = min(M, V) videos as the pair lists of a search; one launch, one workgroup of 256 per
 * query, no workspace.
 * Inputs.  pair_rank [Q][V] int32: smin_video_rank's pair_rank over the (Q, V) scores with pair_ptr[q] = q V (a candidate's rank among
 *   its query's candidates, -1 for a non-candidate).
 * Outputs, every element written.  sel_video [Q][Ms] int32: the videos with 0 <= rank < Ms; a query with fewer than Ms candidates gets
 *   its lowest-indexed non-candidates as well (they yield empty moment lists); ASCENDING BY VIDEO, the order smin_corpus_topk expects
 *   of a query's pairs.  sel_query [Q][Ms] int32 = q.  The videos are scanned in tiles of 256 with running counts (ballot and
 *   popcount, integers only): one writer per slot.  Ranks that are not smin_video_rank's (no permutation of 0 .. candidates - 1) stay
 *   in bounds; slots that find no video then hold -1.
 * Limits.  Q >= 1, 1 <= V <= 0x7fff0000, M >= 1.  Determinism.  The same bits every run.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range or a NULL pointer. */
int smin_prefilter_select(void* stream, const int32_t* pair_rank, int Q, int V, int M, int32_t* sel_video, int32_t* sel_query);

/* smin_window_expand (csrc/window_prune.hip): the (query, window) plan of a pruned window search -- each query's
 * surviving videos expanded to their windows, as SMIN.search_windows expands host pairs sorted by (query, video).  Three launches of
 * workgroups of 256, integers only: a scan of each query's Ms window counts in tiles of 256 (one workgroup per query), a scan of the Q
 * totals in tiles (one workgroup), and the fill (one workgroup per group and ceil(cap / 256) for the padding).  No workgroup waits on
 * another; no atomics, plain stores; no workspace; no host read; capturable.
 * Inputs.  sel_video [Q][Ms] int32: smin_prefilter_select's output, ascending per query; an entry outside [0, V), -1 included, is an
 *   empty group.  video_ptr [V + 1] int64: video v owns windows video_ptr[v] .. video_ptr[v + 1] of a bank of W windows (a pointer
 *   outside [0, W] or below its predecessor is clamped: every window written is a window of the bank).  cap: the slots of the lists.
 * Outputs, every element written.  group_ptr [Q Ms + 1] int64: group g = q Ms + j, the windows of video sel_video[q][j] in start order,
 *   owns slots group_ptr[g] .. group_ptr[g + 1]; the groups in (query, video) order.  win_index [cap], win_query [cap] int32: slot s <
 *   total holds its window, as a global window of the bank, and its query; every slot in [total, cap) holds (0, 0), a real window and
 *   a real query that no group owns.  total [1] int64: the number of real slots, NOT clamped.  total > cap: nothing is written at or
 *   past cap, and every group_ptr entry is clamped to cap (the groups behind own nothing).  group_ptr and total are int64 because
 *   smin_merge_window_moments reads its pair_ptr as int64 (smin_group_pool's int32 copy is made only with the video-level options) and
 *   because Q Ms W passes 2^31 long before cap does.
 * Limits.  Q, Ms, V >= 0, Q Ms <= 0x7f000000, 0 <= W < 2^31, 0 <= cap < 2^31; Ms, Q and a video's window count are not limited to a
 *   tile.  Q Ms == 0: nothing is launched and nothing written.  Determinism.  The same bits every run.
 * Rejection.  A nonzero status before any launch, the outputs untouched, for a size out of range or a NULL pointer (win_index and
 *   win_query may be NULL where cap == 0). */
int smin_window_expand(void* stream, const int32_t* sel_video, const int64_t* video_ptr, int Q, int Ms, int V, int64_t W, int64_t cap,
                       int64_t* group_ptr, int32_t* win_index, int32_t* win_query, int64_t* total);

/* ---- the corpus-wide first-stage cut over shards (csrc/prefilter_fold.hip): smin_prefilter_select's cut of one bank
 * of all the videos, kept as a running best-M per query while the corpus' shards stream past.  wave64, workgroups of 256; no atomics,
 * plain stores; no host read; no allocation; capturable.
 *
 * The order of the cut, a strict total order over a query's videos by their GLOBAL id: candidates (cells > 0) first, among them the
 *   higher first-stage score first by smin_video_rank's comparison (-0 counts as +0; ties go to the lower video); then the
 *   non-candidates in ascending video.  Its first Ms elements are what smin_video_rank + smin_prefilter_select keep of one bank.
 *
 * smin_prefilter_fold: folds one shard into the running state; one launch, one workgroup per query, no workspace.
 * State, read and updated in place, M slots per query:  slot_score [Q][M] fp32, slot_cells [Q][M] fp32 (0: no candidate), slot_video
 *   [Q][M] int32 the global id, -1 for an empty slot.  Invariant: the filled slots are 0 .. n_old - 1 with n_old = min(M, seen).
 * Inputs.  score [Q][Vs], cells [Q][Vs] fp32: smin_prefilter_scores' of the shard; seen: the global id of the shard's video 0 (the
 *   number of videos folded so far); n_old: min(M, seen), stated by the caller and checked.
 * The fold.  n_new = min(M, seen + Vs).  Every element of the union of the n_old old slots and the Vs shard videos gets a 64-bit order
 *   word (distinct ids, distinct words); the words go through LDS 2048 at a time and an element's place is the number of words larger
 *   than its own: no sort, any Vs.  An element stays or is admitted where place < n_new.
 * Slots.  An incumbent that stays keeps its slot: nothing of it is written.  The evicted slots and the empty slots n_old .. n_new - 1,
 *   in ascending slot order, receive the admitted shard videos in ascending local index (two scans with running counts: ballot and
 *   popcount, integers only).  Each slot has one writer.
 * Outputs.  The state: a slot that receives a video gets its score and cells (copied bit for bit) and seen + its local index; slots
 *   >= n_new are written empty (score 0, cells 0, video -1); an incumbent that stays is left alone.  copy_src [Q][M] int32, every
 *   element written: the local index in the shard of the video the slot must receive, -1 to leave the slot alone.
 *   A state that breaks the invariant stays in bounds; its content is then unspecified.
 * Limits.  Q >= 1, 1 <= Vs <= 0x7fff0000, 1 <= M <= 2048, seen >= 0, seen + Vs <= 2^31 - 1.  LDS per workgroup: 42 KB (the slots' words
 *   16 KB, a tile of the shard's 16 KB, the free-slot list 8 KB, the eviction flags 2 KB).  score and cells must not overlap the state
 *   or copy_src.  Work per query: (n_old + Vs)^2 / 256 word comparisons per thread.
 * Determinism.  The same bits every run: places are counts, each slot has one writer.
 * Rejection.  A nonzero status before the launch, the state and copy_src untouched, for a size out of range (M > 2048 among them),
 *   n_old != min(M, seen), seen + Vs past int32 or a NULL pointer. */
int smin_prefilter_fold(void* stream, const float* score, const float* cells, int Q, int Vs, int M, int seen, int n_old, float* slot_score,
                        float* slot_cells, int32_t* slot_video, int32_t* copy_src);

/* smin_survivors_admit: the payload of a fold -- copies the admitted videos of a shard's bank into the bank of survivors; one launch,
 * one workgroup per (row, 32 KB of its fv row).
 * Inputs.  copy_src [R] int32: smin_prefilter_fold's, R = Q M rows (row q M + slot); fv [Vs][T][D] fp32, video_mask [Vs][T], length_mask
 *   [Vs][L], moment_mask [Vs][L][L]: the shard's bank, one byte per mask entry.
 * Outputs.  For every row with 0 <= copy_src[row] < Vs: out_fv [R][T][D] row = the video's fv row (T D floats as float4),
 *   out_video_mask [R][T], out_length_mask [R][L], out_moment_mask [R][L][L] rows = its masks, byte by byte (L L need not be a multiple
 *   of 4), all bit for bit.  Every other row (copy_src -1) is left alone.
 * Limits.  R >= 1, Vs >= 1, T >= 1, 1 <= L <= 4096, D >= 4 with D % 4 == 0, T D / 4 <= 2048 * 65535; fv and out_fv 16-byte aligned.  The
 *   outputs must not overlap the inputs or each other.  Determinism.  Copies: the same bits every run.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size out of range, a NULL pointer or a misaligned fv. */
int smin_survivors_admit(void* stream, const int32_t* copy_src, const float* fv, const uint8_t* video_mask, const uint8_t* length_mask,
                         const uint8_t* moment_mask, int R, int Vs, int T, int L, int D, float* out_fv, uint8_t* out_video_mask,
                         uint8_t* out_length_mask, uint8_t* out_moment_mask);

/* smin_prefilter_gt_rank: the first-stage rank of each query's own video over the whole corpus, O(V) per query (smin_video_rank over
 * the corpus would be O(V^2)); one launch, one workgroup per query.
 * Inputs.  score [Q][V] fp32: the shards' first-stage scores concatenated; cand [V]: one byte per video, nonzero = it has a valid cell
 *   (a video's cell count does not depend on the query); gt_video [Q] int32 or NULL: each query's own video.
 * Output, every element written.  gt_rank [Q] int32: the number of candidates ahead of gt_video[q] in the order above -- the gt_rank
 *   smin_video_rank gives over the (Q, V) scores --; -1 where gt_video is NULL, out of [0, V) (it forms no address before that check)
 *   or no candidate.  Counts per thread (v = t, t + 256, ...) are added over the wave and then the four waves: integers, any order
 *   gives the same value.
 * Limits.  Q >= 1, 1 <= V <= 0x7fff0000.  Rejection.  A nonzero status before the launch, gt_rank untouched, for a size out of range or
 *   a NULL pointer other than gt_video. */
int smin_prefilter_gt_rank(void* stream, const float* score, const uint8_t* cand, const int32_t* gt_video, int Q, int V, int32_t* gt_rank);

/* ---- compact video banks: fv [V][T][D] stored as codes, R = V T rows of D values, decoded by ONE fp32
 * multiplication in front of the arithmetic the fp32 kernels do, so a compact bank gives the bits of an fp32 bank of the decoded values.
 *   SMIN_BANK_BF16: codes [R][D] uint16, the upper half of the fp32 word rounded to nearest even, u' = (u + 0x7fff + ((u >> 16) & 1)) >> 16;
 *     a NaN becomes the quiet NaN 0x7fc0 (the rounding add could carry it to an infinity); decode = bits << 16; no scale (NULL).
 *   SMIN_BANK_INT8: codes [R][D] int8 and scale [R] fp32, per row: amax = max_d |x[d]|, scale = amax / 127.0f and q[d] =
 *     clamp(rintf(x[d] / scale), -127, 127), both divisions correctly rounded (-128 is never produced); amax == 0 gives scale 0 and
 *     codes 0; a row holding a NaN or an infinity gives scale NaN and codes 0 (it decodes to NaN); decode = (float)q * scale.
 * Denormal inputs are not pinned. */
#define SMIN_BANK_BF16 1
#define SMIN_BANK_INT8 2

/* smin_bank_encode: fv [R][D] fp32 -> codes (and scale [R] for SMIN_BANK_INT8; NULL for SMIN_BANK_BF16); one launch, one wave per row:
 * a lane owns the quads lane, lane + 64, ... of the row (float4 loads; one 4-byte (int8) or 8-byte (bf16) store per quad).
 * Arithmetic as above.  The row's amax is a maximum (a butterfly over the wave): any order gives the same bits.
 * Limits.  R >= 1, D >= 4, D % 4 == 0, R D < 2^40; fv 16-byte, codes 8-byte (bf16) or 4-byte (int8) aligned.  No atomics, no host
 * read, capturable.  Determinism.  The same bits every run.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size or mode out of range, a NULL pointer (scale only
 * where the mode has one), a scale given to SMIN_BANK_BF16 or a misaligned pointer. */
int smin_bank_encode(void* stream, const float* fv, int64_t R, int D, int mode, void* codes, float* scale);

/* smin_bank_decode: the decoder alone: out [R][D] fp32 = decode(codes, scale); one launch, one quad per thread.
 * Limits, determinism and rejection as smin_bank_encode (out 16-byte aligned). */
int smin_bank_decode(void* stream, const void* codes, const float* scale, int64_t R, int D, int mode, float* out);

/* smin_pair_assemble_compact: smin_pair_assemble over a compact video bank: f[p][t][:] = decode(codes[vi[p]][t][:]) * fs_bank[qi[p]][:]
 * -- the decode multiplication, then the gate multiplication, each one fp32 product --, fw and fs gathered bit for bit: the bits of
 * smin_pair_assemble on smin_bank_decode's output.  One launch: where D % 16 == 0 a thread takes 16 values of a frame (one 16-byte
 * load of int8 codes, two of bf16) and writes four float4; otherwise one quad per thread.  Both indices are clamped to their banks
 * before they form an address.
 * Limits.  As smin_pair_assemble; codes 16-byte aligned.  No atomics, no host read, capturable; the same bits every run.
 * Rejection.  A nonzero status before the launch, the outputs untouched, for a size or mode out of range, a NULL pointer (scale only
 * where the mode has one) or a misaligned codes pointer. */
int smin_pair_assemble_compact(void* stream, const void* codes, const float* scale, int mode, const float* fs_bank, const float* fw_bank,
                               const int32_t* video_index, const int32_t* query_index, int P, int V, int Q, int T, int Nq, int D, float* f,
                               float* fw, float* fs);

/* smin_prefilter_scores_compact: smin_prefilter_scores with (codes, scale, mode) in place of fv.  Stage 1 is the same contraction
 * with an A-operand loader that decodes four values at a time (csrc/gemm.h PlainMatH / CodeMatQ: an int8 row carries its scale), so the
 * engine is handed the fp32 values of the decoded bank: the bits of smin_prefilter_scores on smin_bank_decode's output, in every
 * mode of smin_set_gemm_mode.  Stage 2 and the workspace (smin_prefilter_ws_bytes) are shared unchanged.
 * Limits and rejection as smin_prefilter_scores, plus the mode and scale rules of smin_bank_encode. */
int smin_prefilter_scores_compact(void* stream, const void* codes, const float* scale, int mode, const float* fs, const float* w,
                                  const float* b, const uint8_t* lmask, const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float tau,
                                  float* score, float* pool, float* cells, float* pm0, float* ps0, float* pe0, void* ws, size_t ws_bytes);

/* smin_survivors_admit_compact: smin_survivors_admit for a compact bank: the admitted videos' code rows (T D esize bytes, 16 at a
 * time where a row's byte count is a multiple of 16, else 4 at a time), their T scales (SMIN_BANK_INT8) and the three masks, bit for bit;
 * rows with copy_src -1 (or naming no video of the shard) are left alone.  One launch, one workgroup per (row, 2048 pieces of its code row).
 * Limits.  As smin_survivors_admit with T D esize / 4 <= 2048 * 65535; codes and out_codes 16-byte aligned.  Rejection.  As smin_survivors_admit, plus the mode and scale rules of smin_bank_encode. */
int smin_survivors_admit_compact(void* stream, const int32_t* copy_src, const void* codes, const float* scale, int mode,
                                 const uint8_t* video_mask, const uint8_t* length_mask, const uint8_t* moment_mask, int R, int Vs, int T, int L,
                                 int D, void* out_codes, float* out_scale, uint8_t* out_video_mask, uint8_t* out_length_mask,
                                 uint8_t* out_moment_mask);

/* ---- stand-alone fp32 MFMA GEMM  C[M][N] = A[M][K] * B[N][K]^T  (used by tests and bench.py's
 * roofline probe; same engine as every contraction above). */
int smin_gemm_nt(void* stream, const float* A, const float* Bm, float* Cm, int M, int N, int K);
/* C += A * B^T through the engine's accumulate epilogue (tests) */
int smin_gemm_nt_acc(void* stream, const float* A, const float* Bm, float* Cm, int M, int N, int K);

#ifdef __cplusplus
}
#endif
#endif /* SMIN_HIP_H */
