// What a run of the one-node core is given, derives and keeps: the state the forward leaves for the backward, the pair banks,
// the flag word, the call value, the saved shape and the dimensions both passes derive.
#pragma once
#include "binding_util.h"

namespace {

// ---------------------------------------------------------------- the state of a run
// Every tensor the forward makes that its backward reads (SminCore::forward saves them in visit_state's order), per SMI layer, per
// LSTM layer and for the whole model.
struct LayerState {
    Tensor fm, hbar, fb, bu, Qb, Kb, P, baq, bqv, A, Hs, chat, cc, ccmean, cum, x1, consts, Wcat;
    std::vector<Tensor> Pcat;
};
struct LstmState { Tensor x, Hout, G, Cs, Wih, Whh; };
struct CoreState {
    Tensor vx, fv, vmaskf, len32, last, f, fw, fs, qmf, lmf, cells, row_ptr, cellmap, Wch_all, what, kb, Mq, uq, shat, pm, psea, fm_out, wb;
    // not among the saved tensors: the tail's vectors (smin_score only), the parameters (saved behind them), the attention maps (outputs)
    Tensor tailv;
    ParamList prm;
    std::vector<Tensor> cmaps, bmaps;
    // smin_forward_pairs only (undefined otherwise): the query bank's sentence features, the pair lists and their CSR groupings.  There
    // fv, vx, vmaskf have a row per video, len32 and the LSTM state a row per query, everything else a row per pair.
    Tensor fs_bank, vi, qi, v_ptr, v_pairs, q_ptr, q_pairs;
    LstmState lstm[2];
    std::vector<LayerState> layer;
};
template <class F>
void visit_state(CoreState& s, F&& fn)
{
    for (Tensor* t : {&s.vx, &s.fv, &s.vmaskf, &s.len32, &s.last, &s.f, &s.fw, &s.fs, &s.qmf, &s.lmf, &s.cells, &s.row_ptr, &s.cellmap, &s.Wch_all, &s.what, &s.kb, &s.Mq,
                      &s.uq, &s.shat, &s.pm, &s.psea, &s.fm_out, &s.wb, &s.fs_bank, &s.vi, &s.qi, &s.v_ptr, &s.v_pairs, &s.q_ptr, &s.q_pairs})
        fn(*t);
    for (auto& l : s.lstm)
        for (Tensor* t : {&l.x, &l.Hout, &l.G, &l.Cs, &l.Wih, &l.Whh}) fn(*t);
    for (auto& l : s.layer) {
        for (Tensor* t : {&l.fm, &l.hbar, &l.fb, &l.bu, &l.Qb, &l.Kb, &l.P, &l.baq, &l.bqv, &l.A, &l.Hs, &l.chat, &l.cc, &l.ccmean, &l.cum, &l.x1, &l.consts, &l.Wcat})
            fn(*t);
        for (auto& p : l.Pcat) fn(p);
    }
}
void size_state(CoreState& s, int64_t nl)
{
    s.layer.resize(nl);
    for (int64_t k = 0; k < nl; ++k) s.layer[k].Pcat.resize((k + 3) / 4);
}
// the state back from what SminCore::forward saved: its tensors in visit_state's order; returns the parameters, saved behind them
ParamList restore_state(CoreState& s, const variable_list& saved, int64_t nl)
{
    size_state(s, nl);
    size_t cursor = 0;
    visit_state(s, [&](Tensor& t) { t = saved[cursor++]; });
    return ParamList(std::vector<Tensor>(saved.begin() + cursor, saved.end()), nl);
}


// smin_score_pairs: the backbone's outputs of V videos and Q queries, each encoded once (smin_encode_videos / smin_encode_queries), and
// the P (video, query) pairs to score: vi / qi [P] int32 on the device.
// smin_forward_pairs (train): no encoded banks -- the run encodes the V videos and Q queries itself (video_features / query_features
// then have a row per video / per query) from the per-video and per-query masks vmask_v / qmask_q, and keeps what the backward needs:
// the CSR groupings of the pairs by video and by query (smin_pair_assemble_bwd).
// A compact video bank (smin_score_pairs_compact; csrc/bank_codec.hip): storage = SMIN_BANK_BF16 / SMIN_BANK_INT8, fv then holds the
// codes (bf16 / int8) and fv_scale the int8 rows' scales (V, T); storage 0 is the fp32 bank.
struct PairBank {
    Tensor fv, fw, fs, vi, qi;
    bool train = false;
    Tensor vmask_v, qmask_q, v_ptr, v_pairs, q_ptr, q_pairs;
    int storage = 0;
    Tensor fv_scale;
};

// The boolean options of the operators (their keyword arguments, named as the SMIN attributes) as one word.
// F_KEEP_ATTENTION: every layer's word-attention maps leave as extra outputs (not differentiable; the backward ignores them):
// the content maps dense (B, L, L, C, Nq), or with F_ATTN_PACKED as packed rows [N*C][Nq] followed by the cellmap; the boundary maps (B, L, Nq)
// F_INPUT_GRADS: video_features / query_features may require grad; the backward then returns their gradients in slots 0 and 1
// (each formed only when autograd asks for it)
enum { F_OVERLAP_BOUNDARY = 1, F_OVERLAP_PREP = 2, F_ASYNC_WEIGHTS = 4, F_BF16_OPERANDS = 8, F_GRAD_SYNC = 16, F_TAIL_SPLIT = 32, F_KEEP_ATTENTION = 64,
       F_ATTN_PACKED = 128, F_INPUT_GRADS = 256, F_PARAM_PREP_KERNEL = 512 };
int64_t flag_word(bool overlap_boundary, bool overlap_prep, bool param_prep_kernel, bool bf16_operand_storage, bool async_weights = false, bool tail_split = false,
                  bool grad_sync = false, bool input_grads = false, bool keep_attention = false, bool attn_packed = false)
{
    return (overlap_boundary ? F_OVERLAP_BOUNDARY : 0) | (overlap_prep ? F_OVERLAP_PREP : 0) | (param_prep_kernel ? F_PARAM_PREP_KERNEL : 0) |
           (bf16_operand_storage ? F_BF16_OPERANDS : 0) | (async_weights ? F_ASYNC_WEIGHTS : 0) | (tail_split ? F_TAIL_SPLIT : 0) | (grad_sync ? F_GRAD_SYNC : 0) |
           (input_grads ? F_INPUT_GRADS : 0) | (keep_attention ? F_KEEP_ATTENTION : 0) | (attn_packed ? F_ATTN_PACKED : 0);
}

// What a run of the core is given, beside video_features, query_features and the parameter list: one value from the operator to
// SminCore::run, through SminCore::apply as a single argument.
struct CoreCall {
    Tensor video_mask, query_mask, length_mask, moment_mask;    // a row per sample; with a bank: per pair (gathered by run_call)
    int64_t T = 0, L = 0, C = 0, nl = 0, maxq = 0, H = 0;
    int64_t flags = 0;
    int64_t n_known = -1;                                       // the number of valid cells of moment_mask when the caller knows it, else -1
    bool scoring = false;                                       // true: forward only (smin_score, smin_score_pairs)
    std::optional<PairBank> bank;
};
enum { N_FIXED = 3 };               // the node's forward arguments ahead of the parameter list: video_features, query_features, the call (one gradient slot each)

// the shape a backward needs beside the saved tensors: every field under its name in ctx->saved_data
struct SavedShape {
    int64_t N, T, L, C, nl, flags, H, Nq_in;
    template <class Self, class F> static void each(Self& s, F fn)
    {
        fn("N", s.N); fn("T", s.T); fn("L", s.L); fn("C", s.C); fn("nl", s.nl); fn("flags", s.flags); fn("H", s.H); fn("Nq_in", s.Nq_in);
    }
    void put(AutogradContext* ctx) const { each(*this, [&](const char* key, int64_t v) { ctx->saved_data[key] = v; }); }
    static SavedShape get(AutogradContext* ctx)
    {
        SavedShape s;
        each(s, [&](const char* key, int64_t& v) { v = ctx->saved_data[key].toInt(); });
        return s;
    }
};

// What both passes derive from a tensor of the batch, the parameters, the shape and the flags
struct Dims {
    at::Device dev;
    at::TensorOptions opt;
    int B, D, Nq, dl, Li, Ci, Ti;
    HStream curs, side;                                         // the caller's stream; the boundary unit's (F_OVERLAP_BOUNDARY, else the caller's)
    Dims(const Tensor& like, int64_t batch, const ParamList& P, int64_t T, int64_t L, int64_t C, int64_t maxq, int64_t flags)
        : dev(like.device()), opt(like.options()), B(i32(batch)), D(i32(P.backbone(P_VE_W).size(0))), Nq(i32(maxq)), dl(i32(P.layer(0, L_CH_W).size(0))), Li(i32(L)),
          Ci(i32(C)), Ti(i32(T)), curs(c10::hip::getCurrentHIPStream(dev.index())), side((flags & F_OVERLAP_BOUNDARY) ? side_stream(dev.index()) : curs) {}
};

}  // namespace
