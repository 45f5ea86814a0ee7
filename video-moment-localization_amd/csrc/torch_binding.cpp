// Torch extension binding of the SMIN hot path: TORCH_LIBRARY(smin_hip, ...) over the C ABI of include/smin_hip.h.
//
// The reference's operator boundary is the nn.Module surface of models.py; below it the drop-in runs as
// ONE library call per forward: smin_hip::smin_forward takes the six forward arguments of SMIN.forward
// (reference models.py:367) plus the module's parameters, shape and switches (by name) and runs the whole model as ONE autograd node
// (SminCore) around the HIP entry points, so the backward pass runs on the autograd engine's thread without the interpreter
// (DistributedDataParallel hooks fire as usual); smin_hip::smin_score is the same forward without a node, for callers that only rank
// (SMIN.score).  smin_forward_pairs and smin_score_pairs are the same two over indexed pairs of videos and queries: every run is
// described by one CoreCall value, and SminCore is the only node (the pair lists travel in the call).  The Python host (video-moment-localization_amd/functional.py, modules.py) binds the
// same C ABI with ctypes, a node per module; it serves the stand-alone sub-module seams and every in-model call that SMIN._plan does not
// send here (SMIN.fused_core = False, inputs that require grad without input_grads, configurations outside the node's limits).
// torch types appear only in this file; libsmin_hip.so knows pointers and sizes.
//
// Only the in-model fast path lives here: the content stream on a mask-driven cell list.
// The operators, their argument checks and TORCH_LIBRARY are here; the rest of the translation unit is in the headers below, in order:
// plumbing, the loss nodes, the core's state and call value, and its two passes as schedules of named stages.
#include "binding_util.h"
#include "loss_nodes.h"
#include "core_state.h"
#include "core_forward.h"
#include "core_backward.h"

namespace {

// ---------------------------------------------------------------- the fused core
// ProposalGeneration + every SMI layer + Localization (models.py:101-126, 306-344) as ONE autograd node: forward and backward
// are schedules of the stages of ForwardPass and BackwardPass, straight-line sequences of the C entry points with hand-placed
// stream forks.  What a node per module (the Python host's graph) pays and this does not: ~60 engine node visits, the engine's
// out-of-place sums for every tensor with several consumers (f_s, f_w, the boundary features, the parameters shared between layers --
// ~45 tiny launches per step), a transposed copy per weight per backward call (one batched launch here) and the autograd bookkeeping
// of the parameter products.
struct SminCore : torch::autograd::Function<SminCore> {
    // The forward pass, for the node's forward (scoring = false: every tensor the backward reads stays in `st`) and for smin_score
    // (scoring = true: forward only -- a layer's tensors are dropped once their last reader is queued, and the last layer ends in
    // smin_score_tail_fwd instead of its content-stream sum, pair product, moment unit and smin_score_map_fwd).
    // Fills st.pm / st.psea, the contiguous parameters st.prm and the attention maps; returns the number of cells.
    // call.bank: the backbone's outputs of the pairs come from banks through smin_pair_assemble and the four masks are the pairs'.
    // Scoring: the banks are given and video_features / query_features are unused.  Training (bank->train): the two
    // encoders run here, once per row of video_features (V, T, Din) and of query_features (Q, words, E), and their state is kept.
    static int64_t run(CoreState& st, const CoreCall& call, const Tensor& video_features, const Tensor& query_features, at::TensorList prm_in)
    {
        const PairBank* bank = call.bank ? &*call.bank : nullptr;
        TORCH_CHECK(!bank || call.scoring != bank->train, "given banks are scored; a training run encodes its own");
        st.prm = ParamList(prm_in, prm_in.size(), call.nl);
        const bool given = bank && !bank->train;
        const Tensor& like = given ? (bank->storage ? bank->fw : bank->fv) : video_features;     // (fp32: its options make the run's tensors)
        const int64_t Tn = given ? bank->fv.size(1) : like.size(1);
        TORCH_CHECK(Tn == call.T, "ProposalGeneration was built for T=", call.T, " but got ", Tn, " frames");
        ForwardPass p(st, call, like, video_features, query_features);
        p.parameter_products();                                 // second stream
        p.prologue();
        p.video_projection();                                   // second stream
        p.backbone();
        p.layout();                                             // the host wait; second stream
        p.word_operands();                                      // second stream
        p.proposal_map();
        for (int64_t k = 0; k < call.nl; ++k) {
            p.gate(k);
            p.boundary_unit(k);                                 // boundary stream
            p.chat(k);
            p.attention(k);
            if (call.scoring && k == call.nl - 1) {             // forward only: the last layer's second half and the score head collapse
                p.score_tail(k);
                return p.N;
            }
            p.clip_mean(k);
            p.moment_unit(k);                                   // joins the boundary stream
            if (call.scoring) {
                // The streams have met (the join above) and every reader of this layer's tensors is queued: all of them go except what the
                // later layers read -- its attention output cc (in `st`), mu, cum and bu (held by fm, cumean, fb), the running gate sum
                LayerState keep;
                keep.cc = st.layer[k].cc;
                st.layer[k] = keep;
            }
        }
        p.score_head();
        return p.N;
    }

    static variable_list forward(AutogradContext* ctx, Tensor video_features, Tensor query_features, const CoreCall& call, at::TensorList prm_in)
    {
        CoreState st;
        const int64_t N = run(st, call, video_features, query_features, prm_in);
        // what backward reads: every tensor of the state, the contiguous parameters, the shape
        variable_list flat;
        visit_state(st, [&](Tensor& t) { flat.push_back(t); });
        for (auto& p : st.prm.all) flat.push_back(p);
        ctx->save_for_backward(flat);
        SavedShape{N, call.T, call.L, call.C, call.nl, call.flags, call.H, query_features.size(1)}.put(ctx);
        // ps / pe / pa leave as three outputs of the node (rows of one buffer), not as selections of one output: the selections'
        // backward nodes cost three zero fills, three copies and two adds between the loss and this node's backward
        variable_list out{st.pm, st.psea[0], st.psea[1], st.psea[2]};
        if (!(call.flags & F_KEEP_ATTENTION)) return out;
        if (call.flags & F_ATTN_PACKED) st.cmaps.push_back(st.cellmap.clone());
        for (auto& t : st.cmaps) out.push_back(t);
        for (auto& t : st.bmaps) out.push_back(t);
        ctx->mark_non_differentiable(variable_list(out.begin() + 4, out.end()));
        return out;
    }

    static variable_list backward(AutogradContext* ctx, variable_list g)
    {
        const SavedShape shape = SavedShape::get(ctx);
        auto sv = ctx->get_saved_variables();
        CoreState st;
        const ParamList P = restore_state(st, sv, shape.nl);
        BackwardPass p(ctx, g, shape, st, P);
        p.transposes();                                         // boundary stream
        p.localization_head();                                  // the boundary heads' half on the boundary stream
        p.accumulators();
        for (int64_t k = shape.nl - 1; k >= 0; --k) p.layer(k);
        p.tail_streams();
        p.word_gradients();                                     // words stream
        p.clip_windows_and_proposal_map();                      // tail stream; main stream
        p.parameter_products();                                 // tail stream
        p.backbone_buffers();
        if (p.pairs) p.pair_assemble();
        p.video_encoder_inputs();
        p.sentence_feature();                                   // the video encoder's weight half on the backbone's weight stream
        for (int layer = 1; layer >= 0; --layer) p.lstm_layer(layer);
        p.input_gradients();
        p.join();
        return p.result();
    }
};

// ---------------------------------------------------------------- the model

// The reference's dataset pads queries and their mask to max_query_length (dataset.py:35, 173); a batch cut to its longest query is
// taken too: the word features are padded in the node as models.py:58-59 does, and the mask here, since every kernel reads max_query_length columns.
Tensor padded_query_mask(const char* op, const Tensor& query_features, const Tensor& query_mask_in, int64_t maxq)
{
    TORCH_CHECK(query_features.dim() == 3, op, ": query_features (B, words, dim)");
    Tensor query_mask = query_mask_in.reshape({query_features.size(0), -1});
    TORCH_CHECK((query_mask.size(1) == query_features.size(1) || query_mask.size(1) == maxq) && query_features.size(1) <= maxq, op, ": query_mask has ",
                query_mask.size(1), " columns for ", query_features.size(1), " words (max_query_length ", maxq, ")");
    if (query_mask.size(1) < maxq) query_mask = at::constant_pad_nd(query_mask, {0, maxq - query_mask.size(1)}, 0);
    return query_mask;
}

// What the four operators over the core share: the device check (`inputs`: every tensor that has to be on the device; the first names
// it), the parameter count, the device guard, the query mask padded to max_query_length, the pairs' masks gathered (call.bank: the
// masks arrive with a row per video / per query), and the run itself -- forward only (call.scoring), else as the node.
variable_list run_call(const char* op, std::initializer_list<const Tensor*> inputs, CoreCall call, const Tensor& video_features, const Tensor& query_features,
                       at::TensorList prm)
{
    for (const Tensor* t : inputs) TORCH_CHECK(t->is_cuda(), op, " runs on a HIP device only (there is no CPU fallback)");
    TORCH_CHECK((int64_t)prm.size() == ParamList::expected(call.nl), op, ": expected ", ParamList::expected(call.nl), " parameters, got ", prm.size());
    c10::hip::HIPGuard device_guard((*inputs.begin())->device().index());
    c10::AutoGradMode grad_mode(!call.scoring && c10::GradMode::is_enabled());
    if (query_features.defined()) call.query_mask = padded_query_mask(op, query_features, call.query_mask, call.maxq);
    if (call.bank) {
        PairBank& bank = *call.bank;
        if (bank.train) { bank.vmask_v = call.video_mask; bank.qmask_q = call.query_mask; }
        // the byte masks per pair: P * (T + Nq + L + L * L) bytes
        call.video_mask = call.video_mask.index_select(0, bank.vi); call.query_mask = call.query_mask.index_select(0, bank.qi);
        call.length_mask = call.length_mask.index_select(0, bank.vi); call.moment_mask = call.moment_mask.index_select(0, bank.vi);
    }
    if (!call.scoring) return SminCore::apply(video_features, query_features, call, prm);
    CoreState st;
    SminCore::run(st, call, video_features, query_features, prm);
    return {st.pm, st.psea[0], st.psea[1], st.psea[2]};
}
using Scores = std::tuple<Tensor, Tensor, Tensor, Tensor>;
Scores scores(const variable_list& out) { return std::make_tuple(out[0], out[1], out[2], out[3]); }

// SMIN.forward (reference models.py:367-377): the six forward arguments, the parameters in SMIN._native_params order, the model's
// shape and, by name, SMIN's switches (SMIN._node_options).  attention: None, or every layer's word-attention maps as well (detached):
// content[k] = ContentAttention.attn_weights (B, L, L, C, Nq) (models.py:207-226) under "dense", or under "packed" the rows [N*C, Nq] of the
// cell list followed by the cellmap (B, L, L) int32 (what SMIN.localize gathers from); boundary[k] = Attention.attn_weights (B, L, Nq)
// (models.py:137-154).  Without attention both lists are empty.
std::tuple<Tensor, Tensor, Tensor, Tensor, std::vector<Tensor>, std::vector<Tensor>> smin_forward(
    const Tensor& video_features, const Tensor& video_mask, const Tensor& query_features, const Tensor& query_mask, const Tensor& length_mask,
    const Tensor& moment_mask, at::TensorList prm, int64_t T, int64_t L, int64_t C, int64_t num_smi_layers, int64_t max_query_length, int64_t lstm_hidden_size,
    bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool async_weights, bool bf16_operand_storage, bool grad_sync,
    std::optional<int64_t> known_cell_count, bool tail_split, bool input_grads, std::optional<c10::string_view> attention)
{
    TORCH_CHECK(input_grads || (!video_features.requires_grad() && !query_features.requires_grad()),
                "smin_forward forms no gradients of video_features / query_features unless input_grads = True (SMIN.input_grads); otherwise inputs that "
                "require grad go through the Python host (SMIN.fused_core = False)");
    const bool packed = attention && *attention == "packed";
    TORCH_CHECK(!attention || packed || *attention == "dense", "smin_forward: attention is None, \"dense\" or \"packed\" (got \"", *attention, "\")");
    const int64_t nl = num_smi_layers;
    const int64_t flags = flag_word(overlap_boundary, overlap_prep, param_prep_kernel, bf16_operand_storage, async_weights, tail_split, grad_sync, input_grads,
                                    attention.has_value(), packed);
    CoreCall call{video_mask, query_mask, length_mask, moment_mask, T, L, C, nl, max_query_length, lstm_hidden_size, flags, known_cell_count.value_or(-1)};
    auto out = run_call("smin_forward", {&video_features}, std::move(call), video_features, query_features, prm);
    const int64_t nc = attention ? nl + (packed ? 1 : 0) : 0, nb = attention ? nl : 0;
    TORCH_CHECK((int64_t)out.size() == 4 + nc + nb, "smin_forward: ", out.size(), " outputs");
    std::vector<Tensor> content(out.begin() + 4, out.begin() + 4 + nc), boundary(out.begin() + 4 + nc, out.end());
    return std::make_tuple(out[0], out[1], out[2], out[3], content, boundary);
}

// SMIN.score: the same model forward only, not an autograd node.  The launches of smin_forward in the same order on
// the same two streams up to the last layer's attention core; then smin_score_tail_fwd.  Outputs as smin_forward's first four.
Scores smin_score(const Tensor& video_features, const Tensor& video_mask, const Tensor& query_features, const Tensor& query_mask, const Tensor& length_mask,
                  const Tensor& moment_mask, at::TensorList prm, int64_t T, int64_t L, int64_t C, int64_t num_smi_layers, int64_t max_query_length, int64_t lstm_hidden_size,
                  bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, std::optional<int64_t> known_cell_count)
{
    const int64_t flags = flag_word(overlap_boundary, overlap_prep, param_prep_kernel, bf16_operand_storage);
    CoreCall call{video_mask, query_mask, length_mask, moment_mask, T, L, C, num_smi_layers, max_query_length, lstm_hidden_size, flags, known_cell_count.value_or(-1), true};
    return scores(run_call("smin_score", {&video_features}, std::move(call), video_features, query_features, prm));
}

// ---- corpus search (SMIN.encode_videos / encode_queries / score_pairs): the two encoders once per video and per
// query, then the model from the Hadamard product on for any list of (video, query) pairs.  Forward only.

// f_v (V, T, D) = the projection with position embedding and mask (models.py:25-36): smin_forward's call with fs == NULL
Tensor smin_encode_videos(const Tensor& video_features, const Tensor& video_mask, at::TensorList prm)
{
    TORCH_CHECK(video_features.is_cuda() && video_mask.is_cuda(), "smin_encode_videos runs on a HIP device only (there is no CPU fallback)");
    at::NoGradGuard no_grad;
    TORCH_CHECK(video_features.dim() == 3 && video_features.scalar_type() == at::kFloat, "smin_encode_videos: video_features float32 (V, T, Din)");
    TORCH_CHECK((int64_t)prm.size() >= P_LSTM, "smin_encode_videos: the parameter list starts with the video encoder's three");
    const int64_t V = video_features.size(0), T = video_features.size(1), Din = video_features.size(2);
    const ParamList P(prm, P_LSTM, 0);
    const Tensor &W = P.backbone(P_VE_W), &bias = P.backbone(P_VE_B), &pe = P.backbone(P_PE);
    const int64_t D = W.size(0);
    TORCH_CHECK(W.dim() == 2 && W.size(1) == Din && bias.numel() == D && pe.dim() == 2 && pe.size(1) == D && pe.size(0) >= T && video_mask.numel() == V * T,
                "smin_encode_videos: shapes of the video encoder's parameters or of video_mask do not fit video_features");
    c10::hip::HIPGuard device_guard(video_features.device().index());
    Tensor vx = cont(video_features.detach());
    Tensor fv = at::empty({V, T, D}, vx.options());
    project_videos(P, vx, video_mask.reshape({V * T}), fv);
    return fv;
}

// (f_w (Q, max_query_length, D), f_s (Q, D)): pack, the two smin_bilstm_layer_fwd calls and smin_sentence_feature_fwd, as smin_forward issues them
std::tuple<Tensor, Tensor> smin_encode_queries(const Tensor& query_features, const Tensor& query_mask_in, at::TensorList prm, int64_t max_query_length,
                                               int64_t lstm_hidden_size)
{
    TORCH_CHECK(query_features.is_cuda() && query_mask_in.is_cuda(), "smin_encode_queries runs on a HIP device only (there is no CPU fallback)");
    at::NoGradGuard no_grad;
    TORCH_CHECK(query_features.scalar_type() == at::kFloat, "smin_encode_queries: query_features float32 (Q, words, dim)");
    TORCH_CHECK((int64_t)prm.size() >= P_LAYER0, "smin_encode_queries: the parameter list starts with the video encoder's three and the LSTM's sixteen");
    Tensor query_mask = padded_query_mask("smin_encode_queries", query_features, query_mask_in, max_query_length);
    c10::hip::HIPGuard device_guard(query_features.device().index());
    LstmState lstm[2];
    auto out = query_encoder(lstm, ParamList(prm, P_LAYER0, 0), query_features.detach(), query_lengths(query_mask), max_query_length, lstm_hidden_size, true);
    return std::make_tuple(out.first, out.second);
}

// SMIN.score_pairs: smin_score for the P pairs (video_index[p], query_index[p]) of banks fv / fw / fs.  The four byte masks are gathered
// per pair, smin_step_prologue runs on the gathered masks, smin_pair_assemble stands where smin_score has its backbone, and from
// "layout, part 2" on it is the code smin_score runs (SminCore::run).  Outputs as smin_score's, one row per pair.
Scores score_pairs_of(const char* op, const Tensor& fv, const std::optional<Tensor>& scale, int storage, const Tensor& fw, const Tensor& fs, const Tensor& video_mask,
                      const Tensor& query_mask_in, const Tensor& length_mask, const Tensor& moment_mask, const Tensor& video_index, const Tensor& query_index,
                      at::TensorList prm, int64_t T, int64_t L, int64_t C, int64_t num_smi_layers, int64_t max_query_length, int64_t lstm_hidden_size, int64_t flags,
                      std::optional<int64_t> known_cell_count)
{
    const int64_t maxq = max_query_length;
    const auto code = storage == 0 ? at::kFloat : storage == SMIN_BANK_BF16 ? at::kBFloat16 : at::kChar;
    TORCH_CHECK(fv.dim() == 3 && fw.dim() == 3 && fs.dim() == 2 && fv.scalar_type() == code && fw.scalar_type() == at::kFloat && fs.scalar_type() == at::kFloat, op,
                ": fv (V, T, D) ", storage == 0 ? "float32" : "bfloat16 (no scale) or int8 (with scale)", ", fw (Q, max_query_length, D), fs (Q, D) float32");
    const int64_t V = fv.size(0), Q = fs.size(0), D = fv.size(2);
    TORCH_CHECK(V >= 1 && Q >= 1 && fv.size(1) == T && fw.size(0) == Q && fw.size(1) == maxq && fw.size(2) == D && fs.size(1) == D && D == 2 * lstm_hidden_size, op,
                ": the banks do not fit each other or the model (T = ", T, ", max_query_length = ", maxq, ", D = ", 2 * lstm_hidden_size, ")");
    TORCH_CHECK(!scale || scale->is_cuda(), op, " runs on a HIP device only (there is no CPU fallback)");
    TORCH_CHECK(!scale || (scale->scalar_type() == at::kFloat && scale->dim() == 2 && scale->size(0) == V && scale->size(1) == T), op,
                ": scale (V, T) float32, one per frame");
    TORCH_CHECK(video_index.dim() == 1 && query_index.dim() == 1 && video_index.size(0) == query_index.size(0) && video_index.size(0) >= 1, op,
                ": video_index and query_index are (P,) with P >= 1");
    TORCH_CHECK(video_mask.size(0) == V && length_mask.size(0) == V && moment_mask.size(0) == V && query_mask_in.size(0) == Q, op,
                ": video_mask, length_mask and moment_mask have a row per video, query_mask a row per query");
    Tensor query_mask = query_mask_in.reshape({Q, -1});
    TORCH_CHECK(query_mask.size(1) == maxq, op, ": query_mask (Q, max_query_length) as the query bank keeps it");
    CoreCall call{video_mask, query_mask, length_mask, moment_mask, T, L, C, num_smi_layers, maxq, lstm_hidden_size, flags, known_cell_count.value_or(-1), true};
    call.bank = PairBank{cont(fv.detach()), cont(fw.detach()), cont(fs.detach()), cont(video_index.to(at::kInt)), cont(query_index.to(at::kInt))};
    call.bank->storage = storage;
    if (scale) call.bank->fv_scale = cont(scale->detach());
    return scores(run_call(op, {&fv, &fw, &fs, &video_mask, &query_mask_in, &length_mask, &moment_mask, &video_index, &query_index}, std::move(call), Tensor(), Tensor(), prm));
}

Scores smin_score_pairs(const Tensor& fv, const Tensor& fw, const Tensor& fs, const Tensor& video_mask, const Tensor& query_mask_in, const Tensor& length_mask,
                        const Tensor& moment_mask, const Tensor& video_index, const Tensor& query_index, at::TensorList prm, int64_t T, int64_t L, int64_t C,
                        int64_t num_smi_layers, int64_t max_query_length, int64_t lstm_hidden_size, bool overlap_boundary, bool overlap_prep, bool param_prep_kernel,
                        bool bf16_operand_storage, std::optional<int64_t> known_cell_count)
{
    return score_pairs_of("smin_score_pairs", fv, std::nullopt, 0, fw, fs, video_mask, query_mask_in, length_mask, moment_mask, video_index, query_index, prm, T, L, C,
                          num_smi_layers, max_query_length, lstm_hidden_size, flag_word(overlap_boundary, overlap_prep, param_prep_kernel, bf16_operand_storage),
                          known_cell_count);
}

// SMIN.score_pairs over a compact video bank: codes (V, T, D) bfloat16 with scale None, or int8 with scale (V, T) float32.
// smin_score_pairs with smin_pair_assemble_compact where it has smin_pair_assemble: the bits of smin_score_pairs on the decoded bank.
Scores smin_score_pairs_compact(const Tensor& codes, const std::optional<Tensor>& scale, const Tensor& fw, const Tensor& fs, const Tensor& video_mask,
                                const Tensor& query_mask_in, const Tensor& length_mask, const Tensor& moment_mask, const Tensor& video_index, const Tensor& query_index,
                                at::TensorList prm, int64_t T, int64_t L, int64_t C, int64_t num_smi_layers, int64_t max_query_length, int64_t lstm_hidden_size,
                                bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, std::optional<int64_t> known_cell_count)
{
    const int storage = scale ? SMIN_BANK_INT8 : SMIN_BANK_BF16;
    return score_pairs_of("smin_score_pairs_compact", codes, scale, storage, fw, fs, video_mask, query_mask_in, length_mask, moment_mask, video_index, query_index, prm,
                          T, L, C, num_smi_layers, max_query_length, lstm_hidden_size, flag_word(overlap_boundary, overlap_prep, param_prep_kernel, bf16_operand_storage),
                          known_cell_count);
}

// moments.corpus_span_topk (SMIN.search_windows' last stage): smin_corpus_span_topk over smin_merge_window_moments'
// lists of G2 (query, video) groups at k_video -- span (G2, k_video, 2) fp32, score (G2, k_video) fp32, window (G2, k_video) int64,
// cell (G2, k_video, 2) int64, count (G2,) int32 --, group_video (G2,) and group_ptr (Q + 1,) int32.  Returns (video (Q, k) int64,
// span (Q, k, 2), score (Q, k), window (Q, k) int64, cell (Q, k, 2) int64, count (Q,) int32), every element written by the kernel.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> corpus_span_topk_op(const Tensor& span, const Tensor& score, const Tensor& window, const Tensor& cell,
                                                                                 const Tensor& count, const Tensor& group_video, const Tensor& group_ptr, int64_t k)
{
    for (const Tensor* t : {&span, &score, &window, &cell, &count, &group_video, &group_ptr})
        TORCH_CHECK(t->is_cuda(), "smin_corpus_span_topk runs on a HIP device only (there is no CPU fallback)");
    for (const Tensor* t : {&span, &score, &window, &cell, &count, &group_video})
        TORCH_CHECK(t->device() == group_ptr.device(), "smin_corpus_span_topk: every tensor on one device");
    const int64_t G2 = span.dim() == 3 ? span.size(0) : -1, kv = span.dim() == 3 ? span.size(1) : -1;
    TORCH_CHECK(G2 >= 0 && G2 < (int64_t(1) << 31) && kv >= 1 && kv <= 64 && span.size(2) == 2 && score.sizes() == at::IntArrayRef({G2, kv}) && window.sizes() == score.sizes() &&
                    cell.sizes() == at::IntArrayRef({G2, kv, 2}) && count.sizes() == at::IntArrayRef({G2}) && group_video.sizes() == count.sizes(),
                "smin_corpus_span_topk: span (G2, k_video, 2), score and window (G2, k_video), cell (G2, k_video, 2), count and group_video (G2,) with 1 <= k_video <= 64");
    TORCH_CHECK(group_ptr.dim() == 1 && group_ptr.size(0) >= 1 && k >= 1 && k <= 64, "smin_corpus_span_topk: group_ptr (Q + 1,) and 1 <= k <= 64");
    TORCH_CHECK(span.scalar_type() == at::kFloat && score.scalar_type() == at::kFloat && window.scalar_type() == at::kLong && cell.scalar_type() == at::kLong &&
                    count.scalar_type() == at::kInt && group_video.scalar_type() == at::kInt && group_ptr.scalar_type() == at::kInt,
                "smin_corpus_span_topk: span and score float32, window and cell int64, count, group_video and group_ptr int32");
    at::NoGradGuard no_grad;
    c10::hip::HIPGuard device_guard(group_ptr.device().index());
    const int64_t Q = group_ptr.size(0) - 1;
    const Tensor sp = cont(span.detach()), sc = cont(score.detach()), wi = cont(window), ce = cont(cell), cn = cont(count), gv = cont(group_video), gp = cont(group_ptr);
    const auto f32 = sp.options(), i64 = wi.options();
    Tensor out_video = at::empty({Q, k}, i64), out_span = at::empty({Q, k, 2}, f32), out_score = at::empty({Q, k}, f32), out_window = at::empty({Q, k}, i64),
           out_cell = at::empty({Q, k, 2}, i64), out_count = at::empty({Q}, cn.options());
    const bool some = G2 > 0;                                   // (no groups: NULL lists, every query comes out empty)
    SMIN_CK(smin_corpus_span_topk(cur(), some ? fp(sp) : nullptr, some ? fp(sc) : nullptr, some ? wi.const_data_ptr<int64_t>() : nullptr,
                                  some ? ce.const_data_ptr<int64_t>() : nullptr, some ? ip(cn) : nullptr, some ? ip(gv) : nullptr, ip(gp), i32(Q), i32(kv), i32(k),
                                  out_video.data_ptr<int64_t>(), fpm(out_span), fpm(out_score), out_window.data_ptr<int64_t>(), out_cell.data_ptr<int64_t>(),
                                  out_count.data_ptr<int32_t>()));
    return std::make_tuple(out_video, out_span, out_score, out_window, out_cell, out_count);
}

// SMIN.forward_pairs: smin_forward for the P pairs (video_index[p], query_index[p]) of V videos and Q queries that
// are each encoded once -- the same autograd node, differentiable with respect to the parameters.  video_features (V, T, Din) and the three
// video-side masks have a row per video, query_features (Q, words, E) and query_mask a row per query; video_index / query_index (P,)
// int32 on the device, and the same pairs grouped by video (v_ptr (V + 1,), v_pairs (P,)) and by query (q_ptr (Q + 1,), q_pairs (P,)),
// each segment in ascending p -- what smin_pair_assemble_bwd sums over.  Outputs as smin_forward's first four, one row per pair.
// No in-node gradient exchange, no input gradients and no attention maps here: those options are not in the schema.
Scores smin_forward_pairs(const Tensor& video_features, const Tensor& video_mask, const Tensor& query_features, const Tensor& query_mask, const Tensor& length_mask,
                          const Tensor& moment_mask, const Tensor& video_index, const Tensor& query_index, const Tensor& v_ptr, const Tensor& v_pairs, const Tensor& q_ptr,
                          const Tensor& q_pairs, at::TensorList prm, int64_t T, int64_t L, int64_t C, int64_t num_smi_layers, int64_t max_query_length,
                          int64_t lstm_hidden_size, bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool async_weights, bool bf16_operand_storage,
                          std::optional<int64_t> known_cell_count, bool tail_split)
{
    TORCH_CHECK(!video_features.requires_grad() && !query_features.requires_grad(), "smin_forward_pairs forms no gradients of video_features / query_features");
    TORCH_CHECK(video_features.dim() == 3 && video_features.scalar_type() == at::kFloat && query_features.dim() == 3 && query_features.scalar_type() == at::kFloat,
                "smin_forward_pairs: video_features (V, T, Din) and query_features (Q, words, E) float32");
    const int64_t V = video_features.size(0), Q = query_features.size(0), P = video_index.numel();
    TORCH_CHECK(V >= 1 && Q >= 1 && P >= 1 && video_index.dim() == 1 && query_index.dim() == 1 && query_index.size(0) == P,
                "smin_forward_pairs: at least one video, one query and one pair; video_index and query_index are (P,)");
    TORCH_CHECK(video_mask.size(0) == V && video_mask.numel() == V * T && length_mask.size(0) == V && moment_mask.size(0) == V,
                "smin_forward_pairs: video_mask (V, T), length_mask and moment_mask have a row per video");
    auto i32list = [](const Tensor& t, int64_t n) { return t.dim() == 1 && t.size(0) == n && t.scalar_type() == at::kInt; };
    TORCH_CHECK(i32list(video_index, P) && i32list(query_index, P) && i32list(v_ptr, V + 1) && i32list(v_pairs, P) && i32list(q_ptr, Q + 1) && i32list(q_pairs, P),
                "smin_forward_pairs: video_index, query_index, v_pairs, q_pairs (P,), v_ptr (V + 1,) and q_ptr (Q + 1,) are int32");
    const int64_t flags = flag_word(overlap_boundary, overlap_prep, param_prep_kernel, bf16_operand_storage, async_weights, tail_split);
    CoreCall call{video_mask, query_mask, length_mask, moment_mask, T, L, C, num_smi_layers, max_query_length, lstm_hidden_size, flags, known_cell_count.value_or(-1)};
    call.bank = PairBank{Tensor(), Tensor(), Tensor(), cont(video_index), cont(query_index), /*train=*/true, Tensor(), Tensor(), cont(v_ptr), cont(v_pairs), cont(q_ptr),
                         cont(q_pairs)};
    auto out = run_call("smin_forward_pairs", {&video_features, &video_mask, &query_features, &query_mask, &length_mask, &moment_mask, &video_index, &query_index, &v_ptr,
                                               &v_pairs, &q_ptr, &q_pairs}, std::move(call), video_features, query_features, prm);
    TORCH_CHECK(out.size() == 4, "smin_forward_pairs: ", out.size(), " outputs");
    return scores(out);
}

Tensor smin_loss(const Tensor& pm, const Tensor& ym, const Tensor& sm, const Tensor& moment_mask, const Tensor& ps, const Tensor& ys, const Tensor& ss, const Tensor& pe,
                 const Tensor& ye, const Tensor& se, const Tensor& pa, const Tensor& ya, const Tensor& length_mask)
{
    TORCH_CHECK(pm.is_cuda(), "smin_loss runs on a HIP device only (there is no CPU fallback)");
    c10::hip::HIPGuard device_guard(pm.device().index());
    return LossNode::apply(pm, ps, pe, pa, ym, sm, moment_mask, ys, ss, ye, se, ya, length_mask);
}

// What the two losses over a pair plan check alike; `extra`: the node's own (P,) operand under its name
void check_pair_loss(const std::string& op, const char* extra_name, const Tensor& pm, const Tensor& ps, const Tensor& pe, const Tensor& moment_mask, const Tensor& q_ptr,
                     const Tensor& q_pairs, const Tensor& extra)
{
    for (const Tensor* t : {&pm, &ps, &pe, &moment_mask, &q_ptr, &q_pairs, &extra}) TORCH_CHECK(t->is_cuda(), op, " runs on a HIP device only (there is no CPU fallback)");
    for (const Tensor* t : {&ps, &pe, &moment_mask, &q_ptr, &q_pairs, &extra}) TORCH_CHECK(t->device() == pm.device(), op, ": every tensor on one device");
    const int64_t P = pm.dim() == 3 ? pm.size(0) : -1, L = pm.dim() == 3 ? pm.size(1) : -1;
    TORCH_CHECK(P >= 1 && L >= 1 && pm.size(2) == L && ps.sizes() == at::IntArrayRef({P, L}) && pe.sizes() == ps.sizes() && moment_mask.sizes() == pm.sizes(), op,
                ": pm (P, L, L), ps (P, L), pe (P, L) and moment_mask (P, L, L) with P, L >= 1");
    TORCH_CHECK(q_ptr.dim() == 1 && q_ptr.size(0) >= 2 && q_pairs.dim() == 1 && q_pairs.size(0) == P && extra.dim() == 1 && extra.size(0) == P, op,
                ": q_ptr (Q + 1,) with Q >= 1, q_pairs (P,) and ", extra_name, " (P,)");
}

// training.pair_rank_loss: the contrastive term over a pair plan's P pairs (PairRankNode, loss_nodes.h); gradients to pm, ps, pe only
std::tuple<Tensor, Tensor, Tensor> smin_pair_rank_loss(const Tensor& pm, const Tensor& ps, const Tensor& pe, const Tensor& moment_mask, const Tensor& q_ptr,
                                                       const Tensor& q_pairs, const Tensor& positive, double tau, double gamma)
{
    check_pair_loss("smin_pair_rank_loss", "positive", pm, ps, pe, moment_mask, q_ptr, q_pairs, positive);
    TORCH_CHECK(std::isfinite(tau) && tau > 0 && std::isfinite(gamma) && gamma > 0, "smin_pair_rank_loss: tau and gamma must be finite and positive");
    c10::hip::HIPGuard device_guard(pm.device().index());
    auto out = PairRankNode::apply(pm, ps, pe, moment_mask, q_ptr, q_pairs, positive, tau, gamma);
    return std::make_tuple(out[0], out[1], out[2]);
}

// training.pair_distill_loss: the soft-target term over a pair plan's P pairs (PairDistillNode, loss_nodes.h); gradients to pm, ps, pe only
std::tuple<Tensor, Tensor, Tensor> smin_pair_distill_loss(const Tensor& pm, const Tensor& ps, const Tensor& pe, const Tensor& moment_mask, const Tensor& q_ptr,
                                                          const Tensor& q_pairs, const Tensor& teacher, double tau, double gamma, double gamma_teacher)
{
    check_pair_loss("smin_pair_distill_loss", "teacher", pm, ps, pe, moment_mask, q_ptr, q_pairs, teacher);
    TORCH_CHECK(std::isfinite(tau) && tau > 0 && std::isfinite(gamma) && gamma > 0 && std::isfinite(gamma_teacher) && gamma_teacher > 0,
                "smin_pair_distill_loss: tau, gamma and gamma_teacher must be finite and positive");
    c10::hip::HIPGuard device_guard(pm.device().index());
    auto out = PairDistillNode::apply(pm, ps, pe, moment_mask, q_ptr, q_pairs, teacher, tau, gamma, gamma_teacher);
    return std::make_tuple(out[0], out[1], out[2]);
}

// FusedAdam.step (optim.py): the pointers of the parameters and their gradients are gathered here -- with
// zero_grad(set_to_none=True) the gradients move every step -- and handed to smin_grad_norm (when clipping or the guard is on) and
// smin_adam_step on the current stream.  No host read: capturable as it stands, the pointers baked into the graph as for torch's own
// fused Adam.  max_norm < 0: no clipping.  ws: the norm's partials (uint8, smin_adam_ws_bytes), required when the norm runs.
void adam_step(at::TensorList params, at::TensorList grads, const Tensor& exp_avg_flat, const Tensor& exp_avg_sq_flat, at::IntArrayRef offsets,
               const Tensor& state, const std::optional<Tensor>& ws, double beta1, double beta2, double eps, double weight_decay, bool decoupled,
               double max_norm, bool skip_nonfinite)
{
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && offsets.size() == n, "adam_step: ", n, " parameters, ", grads.size(), " gradients, ", offsets.size(), " offsets");
    TORCH_CHECK(exp_avg_flat.is_cuda(), "adam_step runs on a HIP device only (there is no CPU fallback)");
    const auto dev = exp_avg_flat.device();
    auto flat_ok = [&](const Tensor& t, at::ScalarType ty) { return t.device() == dev && t.scalar_type() == ty && t.is_contiguous(); };
    TORCH_CHECK(flat_ok(exp_avg_flat, at::kFloat) && flat_ok(exp_avg_sq_flat, at::kFloat) && exp_avg_flat.numel() == exp_avg_sq_flat.numel(),
                "adam_step: the moment buffers must be contiguous fp32 tensors of one size on one HIP device");
    TORCH_CHECK(flat_ok(state, at::kDouble) && state.numel() == 8, "adam_step: state must be 8 contiguous doubles on the parameters' device");
    std::vector<float*> pp(n);
    std::vector<const float*> gp(n);
    std::vector<int64_t> ne(n), mo(n);
    int64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const Tensor &p = params[i], &g = grads[i];
        TORCH_CHECK(p.is_cuda() && g.is_cuda(), "adam_step runs on a HIP device only (there is no CPU fallback): parameter ", i);
        TORCH_CHECK(p.device() == dev && g.device() == dev, "adam_step: parameter ", i, " or its gradient is on another device");
        TORCH_CHECK(p.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat, "adam_step: parameter ", i, " or its gradient is not fp32");
        TORCH_CHECK(p.is_contiguous() && g.is_contiguous(), "adam_step: parameter ", i, " or its gradient is not contiguous");
        TORCH_CHECK(p.sizes() == g.sizes(), "adam_step: gradient ", i, " has not its parameter's shape");
        ne[i] = p.numel();
        mo[i] = offsets[i];
        TORCH_CHECK(mo[i] >= 0 && mo[i] + ne[i] <= exp_avg_flat.numel(), "adam_step: moment segment ", i, " lies outside the flat buffers");
        pp[i] = p.numel() ? p.data_ptr<float>() : nullptr;
        gp[i] = g.numel() ? g.const_data_ptr<float>() : nullptr;
        total += ne[i];
        torch::autograd::impl::bump_version(p);                   // written in place below, as far as autograd's saved tensors are concerned
    }
    const bool norm = max_norm >= 0.0 || skip_nonfinite;
    c10::hip::HIPGuard device_guard(dev.index());
    void* wsp = nullptr;
    if (norm) {
        const size_t need = smin_adam_ws_bytes(total, i32((int64_t)n));
        TORCH_CHECK(ws && ws->defined() && ws->device() == dev && ws->scalar_type() == at::kByte && ws->is_contiguous() && (size_t)ws->numel() >= need,
                    "adam_step: the norm needs a uint8 workspace of ", need, " bytes on the parameters' device");
        wsp = ws->data_ptr();
        SMIN_CK(smin_grad_norm(cur(), gp.data(), ne.data(), i32((int64_t)n), max_norm >= 0.0 ? max_norm : -1.0, state.data_ptr<double>(), wsp,
                               (size_t)ws->numel()));
    }
    SMIN_CK(smin_adam_step(cur(), pp.data(), gp.data(), ne.data(), mo.data(), i32((int64_t)n), exp_avg_flat.data_ptr<float>(),
                           exp_avg_sq_flat.data_ptr<float>(), state.data_ptr<double>(), beta1, beta2, eps, weight_decay, decoupled ? 1 : 0,
                           skip_nonfinite ? 1 : 0, wsp));
}

}  // namespace

TORCH_LIBRARY(smin_hip, m)
{
    // SMIN.forward as one autograd node (see smin_forward above)
    m.def("smin_forward(Tensor video_features, Tensor video_mask, Tensor query_features, Tensor query_mask, Tensor length_mask, Tensor moment_mask, "
          "Tensor[] params, int T, int L, int C, int num_smi_layers, int max_query_length, int lstm_hidden_size, *, bool overlap_boundary, "
          "bool overlap_prep, bool param_prep_kernel, bool async_weights, bool bf16_operand_storage, bool grad_sync, int? known_cell_count, "
          "bool tail_split, bool input_grads, str? attention) -> (Tensor, Tensor, Tensor, Tensor, Tensor[], Tensor[])", &smin_forward);
    // SMIN.score: the forward-only scoring path, the last layer collapsed to row dots (see smin_score above)
    m.def("smin_score(Tensor video_features, Tensor video_mask, Tensor query_features, Tensor query_mask, Tensor length_mask, Tensor moment_mask, "
          "Tensor[] params, int T, int L, int C, int num_smi_layers, int max_query_length, int lstm_hidden_size, *, bool overlap_boundary, "
          "bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, int? known_cell_count) -> (Tensor, Tensor, Tensor, Tensor)", &smin_score);
    // corpus search: the two encoders alone, and smin_score over indexed pairs of their banks
    m.def("smin_encode_videos(Tensor video_features, Tensor video_mask, Tensor[] params) -> Tensor", &smin_encode_videos);
    m.def("smin_encode_queries(Tensor query_features, Tensor query_mask, Tensor[] params, int max_query_length, int lstm_hidden_size) -> (Tensor, Tensor)",
          &smin_encode_queries);
    m.def("smin_score_pairs(Tensor fv, Tensor fw, Tensor fs, Tensor video_mask, Tensor query_mask, Tensor length_mask, Tensor moment_mask, Tensor video_index, "
          "Tensor query_index, Tensor[] params, int T, int L, int C, int num_smi_layers, int max_query_length, int lstm_hidden_size, *, bool overlap_boundary, "
          "bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, int? known_cell_count) -> (Tensor, Tensor, Tensor, Tensor)", &smin_score_pairs);
    // the same over a compact video bank: bf16 codes, or int8 codes and the frames' scales
    m.def("smin_score_pairs_compact(Tensor codes, Tensor? scale, Tensor fw, Tensor fs, Tensor video_mask, Tensor query_mask, Tensor length_mask, Tensor moment_mask, "
          "Tensor video_index, Tensor query_index, Tensor[] params, int T, int L, int C, int num_smi_layers, int max_query_length, int lstm_hidden_size, *, "
          "bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, int? known_cell_count) -> (Tensor, Tensor, Tensor, Tensor)",
          &smin_score_pairs_compact);
    // SMIN.search_windows' ranking across videos: span-valued moments of (query, video) groups into one list per query
    m.def("smin_corpus_span_topk(Tensor span, Tensor score, Tensor window, Tensor cell, Tensor count, Tensor group_video, Tensor group_ptr, int k) -> "
          "(Tensor video, Tensor span, Tensor score, Tensor window, Tensor cell, Tensor count)", &corpus_span_topk_op);
    // SMIN.forward_pairs: smin_forward over indexed pairs of videos and queries encoded once each, one autograd node
    m.def("smin_forward_pairs(Tensor video_features, Tensor video_mask, Tensor query_features, Tensor query_mask, Tensor length_mask, Tensor moment_mask, "
          "Tensor video_index, Tensor query_index, Tensor v_ptr, Tensor v_pairs, Tensor q_ptr, Tensor q_pairs, Tensor[] params, int T, int L, int C, "
          "int num_smi_layers, int max_query_length, int lstm_hidden_size, *, bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, "
          "bool async_weights, bool bf16_operand_storage, int? known_cell_count, bool tail_split) -> (Tensor, Tensor, Tensor, Tensor)", &smin_forward_pairs);
    // restated loss_fn of the reference's train loop (main.py:110-116), same argument order
    m.def("smin_loss(Tensor pm, Tensor ym, Tensor sm, Tensor moment_mask, Tensor ps, Tensor ys, Tensor ss, Tensor pe, Tensor ye, Tensor se, Tensor pa, Tensor ya, "
          "Tensor length_mask) -> Tensor", &smin_loss);
    // the contrastive term beside smin_loss: each query's own video ranked above the wrong ones of its pair plan
    m.def("smin_pair_rank_loss(Tensor pm, Tensor ps, Tensor pe, Tensor moment_mask, Tensor q_ptr, Tensor q_pairs, Tensor positive, float tau, float gamma) -> "
          "(Tensor loss, Tensor stats, Tensor pair_score)", &smin_pair_rank_loss);
    // the soft-target term beside it: each query's softmax over its pairs pulled towards a teacher's scores of them
    m.def("smin_pair_distill_loss(Tensor pm, Tensor ps, Tensor pe, Tensor moment_mask, Tensor q_ptr, Tensor q_pairs, Tensor teacher, float tau, float gamma, "
          "float gamma_teacher) -> (Tensor loss, Tensor stats, Tensor pair_score)", &smin_pair_distill_loss);
    // FusedAdam.step: Adam / AdamW over a parameter list, gradient norm, clipping and the non-finite guard on the device (see adam_step above)
    m.def("adam_step(Tensor[] params, Tensor[] grads, Tensor exp_avg_flat, Tensor exp_avg_sq_flat, int[] offsets, Tensor state, Tensor? ws, float beta1, "
          "float beta2, float eps, float weight_decay, bool decoupled, float max_norm, bool skip_nonfinite) -> ()", &adam_step);
    m.def("abi_version() -> int", []() -> int64_t { return smin_abi_version(); });
    // the status word of smin_build_cells_n on a device (non-zero after a step whose known_cell_count did not match its mask)
    m.def("layout_status(Device device) -> Tensor", [](c10::Device dev) { return layout_status(dev); });
    // data parallel: the process group (c10d group name) the one-node backward averages its gradients over, see GradSync;
    // smin_forward's grad_sync switches the exchange on per call.  coalesced_avg: the backend takes grouped "avg" all-reduces (RCCL)
    m.def("set_grad_sync(str group_name, int world, bool coalesced_avg) -> ()", [](std::string group, int64_t world, bool coalesced_avg) {
        GradSyncConfig& c = grad_sync_config();
        c.group = std::move(group); c.world = (int)world; c.coalesced_avg = coalesced_avg;
    });
}
