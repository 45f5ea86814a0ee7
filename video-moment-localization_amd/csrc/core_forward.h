// The two encoders of the backbone, and the forward pass of the one-node core as a schedule of stages (SminCore::run lists them in order).
#pragma once
#include "core_state.h"

namespace {

// What smin_encode_queries / smin_encode_videos and a training run over pairs (SminCore::run) both do: the lengths of a (Q, words) mask;
// a (V * T) video mask as fp32 (returned) and the video encoder's projection f_v (models.py:25-36) of the V videos into `fv`
Tensor query_lengths(const Tensor& query_mask) { return query_mask.ne(0).sum(1).to(at::kInt).contiguous(); }
Tensor project_videos(const ParamList& P, const Tensor& vx, const Tensor& video_mask, const Tensor& fv)
{
    Tensor vmaskf = cont(video_mask.is_floating_point() ? fl(video_mask) : video_mask.ne(0).to(at::kFloat));
    SMIN_CK(smin_video_encoder_fwd(cur(), fp(vx), fp(P.backbone(P_VE_W)), fp(P.backbone(P_VE_B)), fp(P.backbone(P_PE)), fp(vmaskf), nullptr, i32(vx.size(0)), i32(vx.size(1)),
                                   i32(vx.size(2)), i32(fv.size(2)), fpm(fv), nullptr));
    return vmaskf;
}

// The query encoder (models.py:38-62): both BiLSTM layers' operand layouts in one launch, the two recurrences, f_w padded to
// max_query_length and the sentence feature f_s.  The layers' tensors that a backward reads stay in `lstm` (scoring: dropped).
std::pair<Tensor, Tensor> query_encoder(LstmState (&lstm)[2], const ParamList& P, const Tensor& query_features, const Tensor& len32, int64_t maxq,
                                        int64_t H, bool scoring)
{
    const auto opt = query_features.options();
    Tensor x = cont(query_features);
    const int64_t Bq = x.size(0), Nq_in = x.size(1);
    const int B = i32(Bq);
    // both layers' operand layouts in one launch, ahead of the first recurrence (a launch per layer sat between the two)
    Tensor lstm_bias[2], lstm_W4[2];
    {
        const float* raw[16]; int ins[2]; float *wih[2], *bs[2], *whh[2], *w4[2];
        for (int layer = 0; layer < 2; ++layer) {
            LstmState& ls = lstm[layer];
            const int64_t In = layer == 0 ? x.size(2) : 2 * H;
            ls.Wih = at::empty({8 * H, In}, opt);                              // [w_ih; w_ih_reverse]
            lstm_bias[layer] = at::empty({8 * H}, opt);                        // b_ih + b_hh per direction
            ls.Whh = at::empty({2, 4 * H, H}, opt);
            lstm_W4[layer] = at::empty({2, H, H, 4}, opt);                     // [d, k, u, gate]
            for (int q = 0; q < 8; ++q) raw[8 * layer + q] = fp(P.backbone(P_LSTM + 8 * layer + q));
            ins[layer] = i32(In); wih[layer] = fpm(ls.Wih); bs[layer] = fpm(lstm_bias[layer]); whh[layer] = fpm(ls.Whh); w4[layer] = fpm(lstm_W4[layer]);
        }
        SMIN_CK(smin_lstm_pack_layers(cur(), 2, raw, ins, i32(H), wih, bs, whh, w4));
    }
    for (int layer = 0; layer < 2; ++layer) {
        LstmState& ls = lstm[layer];
        const int In = i32(x.size(2)), Hh = i32(H);
        ls.x = x;
        const Tensor &bias = lstm_bias[layer], &W4 = lstm_W4[layer];
        ls.G = at::empty({Bq, Nq_in, 2, 4 * H}, opt); ls.Hout = at::empty({Bq, Nq_in, 2 * H}, opt); ls.Cs = at::empty({Bq, Nq_in, 2, H}, opt);
        SMIN_CK(smin_bilstm_layer_fwd(cur(), fp(x), fp(ls.Wih), fp(bias), fp(W4), ip(len32), B, i32(Nq_in), In, Hh, fpm(ls.G), fpm(ls.Hout), fpm(ls.Cs)));
        x = ls.Hout;
    }
    if (scoring)                                                               // (main-stream tensors that only the backward reads)
        for (auto& l : lstm) { l.G = Tensor(); l.Cs = Tensor(); }
    Tensor fw = x;
    if (Nq_in < maxq) fw = at::constant_pad_nd(fw, {0, 0, 0, maxq - Nq_in}, 0);
    fw = fw.contiguous();
    Tensor fs = at::empty({Bq, 2 * H}, opt);                                    // [h_fwd at the last word | h_bwd at the first word]
    SMIN_CK(smin_sentence_feature_fwd(cur(), fp(fw), ip(len32), B, i32(fw.size(1)), i32(H), fpm(fs)));
    return {fw, fs};
}

// ---------------------------------------------------------------- the forward pass
// ProposalGeneration + every SMI layer + Localization (models.py:101-126, 306-344) as a schedule of stages on two streams: the
// caller's (`curs`) and a second one (`prep` for parameter-only work, `side` for the boundary unit; one stream, or the caller's when
// the option is off).  SminCore::run lists the stages in order.  The members are what outlives a stage: the events of the hand-offs,
// each marked by the stage that produces and awaited by the stage that first consumes, and every tensor that a later stage or the other
// stream reads and `st` does not hold.  Tensors cross streams without recordStream bookkeeping: DESIGN.md 6, "Stream rules" (4) says
// what makes that safe, for scoring's early release of a layer's tensors too.
struct ForwardPass : Dims {
    CoreState& st;
    const CoreCall& call;
    const Tensor &video_features, &query_features;
    const PairBank* const bank;                                 // the call's banks, or null
    const bool own_bank;                                        // a training run over pairs: it encodes its own banks
    const ParamList& P;                                         // st.prm
    const int64_t T, L, C, nl, maxq, H, flags, n_known, Bq;
    const bool scoring;
    const HStream prep;
    // Tensors that only ever feed contractions (the pair product, the attention outputs cc_k) are stored as bf16 when the contractions
    // round their operands to bf16 anyway (smin_set_gemm_mode(2)): no bit of the step changes, half the bytes
    const bool bf16_operands, cc_bf16, keep_maps;
    hipEvent_t products_ready = nullptr, count_ready = nullptr, projection_ready = nullptr, layout_ready = nullptr, words_ready = nullptr;
    std::vector<Tensor> bcat;                                   // per layer: the moment unit's two biases summed
    Tensor bb, qm, mm, host_n, mask8, pgs;                      // the boundary heads' biases; masks and the cell count; every layer's clip-window term of chat
    int64_t N = 0;                                              // the number of cells (layout)
    int n = 0;
    Tensor fm, fb, cumean, Hs;                                  // running: the layer's inputs, mean_c f_c, the sum of the earlier layers' gated features

    ForwardPass(CoreState& st, const CoreCall& call, const Tensor& like, const Tensor& video_features, const Tensor& query_features)
        : Dims(like, call.bank ? call.bank->vi.size(0) : video_features.size(0), st.prm, call.T, call.L, call.C, call.maxq, call.flags), st(st), call(call),
          video_features(video_features), query_features(query_features), bank(call.bank ? &*call.bank : nullptr), own_bank(bank && bank->train), P(st.prm), T(call.T),
          L(call.L), C(call.C), nl(call.nl), maxq(call.maxq), H(call.H), flags(call.flags), n_known(call.n_known), Bq(B), scoring(call.scoring),
          prep((flags & F_OVERLAP_PREP) ? side : curs), bf16_operands((flags & F_BF16_OPERANDS) && smin_get_gemm_mode() == 2), cc_bf16(bf16_operands && dl % 8 == 0),
          keep_maps((flags & F_KEEP_ATTENTION) != 0), bcat(nl)
    {
        size_state(st, nl);
    }

    // ---- parameter-only work (weight products, constants, concatenations: ~25 tiny launches) on the second stream from the first
    // moment of the step, beside the LSTM recurrence that opens the critical path; the main stream waits for it before the proposal map
    void parameter_products()
    {
        const bool prep_kernel = (flags & F_PARAM_PREP_KERNEL) != 0;                // csrc/param_prep.hip (else: torch calls)
        wait_stream(prep, curs);                                                    // (the optimizer's update of the parameters)
        StreamScope sc(prep);
        if (prep_kernel) {
            Tensor consts_all = at::empty({nl, dl}, opt), Wcat_all = at::empty({nl, D, 2 * D}, opt), bcat_all = at::empty({nl, D}, opt);
            st.Wch_all = at::empty({nl * dl, D}, opt);
            std::vector<const float*> pp;
            std::vector<float*> pc(nl * 2, nullptr);
            for (int64_t k = 0; k < nl; ++k) {
                for (int which : L_PRODUCTS) pp.push_back(fp(P.layer(k, which)));
                LayerState& ls = st.layer[k];
                for (int64_t lo = 0; lo < k; lo += 4) {
                    ls.Pcat[lo / 4] = at::empty({dl, std::min<int64_t>(4, k - lo) * dl}, opt);
                    pc[k * 2 + lo / 4] = fpm(ls.Pcat[lo / 4]);
                }
                ls.consts = consts_all[k]; ls.Wcat = Wcat_all[k]; bcat[k] = bcat_all[k];
            }
            SMIN_CK(smin_param_prep_fwd(cur(), pp.data(), i32(nl), D, dl, pc.data(), fpm(consts_all), fpm(Wcat_all), fpm(bcat_all), fpm(st.Wch_all)));
        } else {
            Tensor bsum;
            std::vector<Tensor> wch;
            for (int64_t k = 0; k < nl; ++k) {
                LayerState& ls = st.layer[k];
                ls.consts = bsum.defined() ? P.layer(k, L_CH_B) + at::mv(P.layer(k, L_CH_W), bsum) : P.layer(k, L_CH_B);
                bsum = bsum.defined() ? bsum + P.layer(k, L_C_B) : P.layer(k, L_C_B);
                wch.push_back(P.layer(k, L_CH_W));
                for (int64_t lo = 0; lo < k; lo += 4) {
                    std::vector<Tensor> parts;
                    for (int64_t l = lo; l < std::min(lo + 4, k); ++l) parts.push_back(at::matmul(P.layer(k, L_CH_W), P.layer(l, L_C_W)));
                    ls.Pcat[lo / 4] = parts.size() == 1 ? parts[0] : at::cat(parts, 1);
                }
                ls.Wcat = at::cat({P.layer(k, L_FB_W).view({D, D}), P.layer(k, L_FC_W).view({D, D})}, 1);
                bcat[k] = P.layer(k, L_FB_B) + P.layer(k, L_FC_B);
            }
            st.Wch_all = nl == 1 ? wch[0] : at::cat(wch);
        }
        if (scoring) {
            // the forward-only tail's vectors (csrc/score_tail.hip): parameters only, so here, beside the LSTM, not in front of the tail
            const int64_t k = nl - 1;
            st.tailv = at::empty({(int64_t)smin_score_tail_ws_bytes(B, Li, D, dl)}, opt.dtype(at::kByte));
            SMIN_CK(smin_score_tail_fwd(cur(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, B, Li, D, dl, fp(P.layer(k, L_C_W)), fp(P.layer(k, L_C_B)),
                                        fp(st.layer[k].Wcat), fp(bcat[k]), fp(P.loc(0)), fp(P.loc(1)), nullptr, nullptr, nullptr, nullptr, nullptr, st.tailv.data_ptr(),
                                        (size_t)st.tailv.numel()));
        }
        products_ready = mark(prep);
    }

    // ---- masks as fp32, query lengths, the cell count, the boundary heads' parameters side by side: one launch (csrc/layout.hip);
    // as torch calls (masks that are not one byte per element) eight launches in front of the query encoder
    void prologue()
    {
        const Tensor &video_mask = call.video_mask, &query_mask = call.query_mask, &length_mask = call.length_mask, &moment_mask = call.moment_mask;
        qm = query_mask.reshape({Bq, -1});
        auto bytes = [](const Tensor& t) { return t.element_size() == 1 && t.is_contiguous(); };
        const bool fast_prologue = bytes(video_mask) && bytes(qm) && bytes(length_mask) && bytes(moment_mask) && qm.size(1) == maxq && video_mask.numel() == Bq * T &&
                                   length_mask.numel() == Bq * L && moment_mask.numel() == Bq * L * L;
        if (fast_prologue) {
            st.wb = at::empty({3, (int64_t)D}, opt); bb = at::empty({3}, opt);
            st.len32 = at::empty({Bq}, opt.dtype(at::kInt));
            st.qmf = at::empty({Bq, maxq}, opt); st.lmf = at::empty({Bq, L}, opt); st.vmaskf = at::empty({Bq * T}, opt);
            Tensor count = at::empty({1}, opt.dtype(at::kLong));
            const float* w3[3] = {fp(P.loc(2)), fp(P.loc(4)), fp(P.loc(6))};
            const float* b3[3] = {fp(P.loc(3)), fp(P.loc(5)), fp(P.loc(7))};
            SMIN_CK(smin_step_prologue(cur(), u8(qm), u8(video_mask), u8(length_mask), u8(moment_mask), w3, b3, B, Nq, Ti, Li, D, st.len32.data_ptr<int32_t>(), fpm(st.qmf),
                                       fpm(st.vmaskf), fpm(st.lmf), fpm(st.wb), fpm(bb), count.data_ptr<int64_t>(), prologue_words(dev).data_ptr()));
            mm = moment_mask;
            if (n_known < 0) {
                host_n = at::empty({1}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
                host_n.copy_(count, /*non_blocking=*/true);
            }
        } else {
            st.wb = at::stack({P.loc(2).view({D}), P.loc(4).view({D}), P.loc(6).view({D})});
            bb = at::cat({P.loc(3), P.loc(5), P.loc(7)});
            // ---- layout, part 1: the cell count leaves for the host now and is waited for after the backbone is queued -- unless the
            // caller already knows it (n_known; a captured step: nothing inside may wait for the device)
            mm = moment_mask.scalar_type() == at::kBool ? moment_mask : moment_mask.ne(0);
            if (n_known < 0) {
                host_n = at::empty({1}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
                host_n.copy_(mm.sum().reshape({1}), /*non_blocking=*/true);
            }
            st.len32 = qm.sum(1).to(at::kInt);
            st.vmaskf = cont(fl(video_mask.reshape({Bq * T})));
            st.qmf = cont(fl(qm)); st.lmf = cont(fl(length_mask));
        }
        count_ready = mark(curs);
    }

    // ---- the video encoder's projection (models.py:25-36) on the second stream, beside the query encoder: only its product with the
    // sentence feature (models.py:81-83) waits for the LSTM layers (the fused call sat behind them: ~90 us of the step's opening chain).
    // Queued behind the parameter products: ahead of them it runs beside the LSTM operand packing and the first recurrence and
    // stretches both (pack 20 -> 84 us, recurrence 87 -> 130 us: the opening chain 45 us longer, tools/gantt.sh).
    void video_projection()
    {
        if (!bank || own_bank) {
            st.vx = cont(video_features);
            st.fv = at::empty({st.vx.size(0), T, (int64_t)D}, opt);
        }
        st.f = at::empty({Bq, T, (int64_t)D}, opt);
        if (!bank && prep != curs) {
            await(prep, count_ready);                                              // (vmaskf)
            StreamScope sc(prep);
            SMIN_CK(smin_video_encoder_fwd(cur(), fp(st.vx), fp(P.backbone(P_VE_W)), fp(P.backbone(P_VE_B)), fp(P.backbone(P_PE)), fp(st.vmaskf), nullptr, B, Ti,
                                           i32(st.vx.size(2)), D, fpm(st.fv), nullptr));
            projection_ready = mark(prep);
        }
    }

    // ---- backbone (models.py:38-83): BiLSTM x 2, sentence feature, fused video encoder; or the pairs' rows from banks, given or its own
    void backbone()
    {
        if (bank) {
            Tensor bfv = bank->fv, bfw = bank->fw, bfs = bank->fs;
            if (own_bank) {
                // the two encoders once per video and once per query, on the main stream (as smin_encode_videos / smin_encode_queries);
                // the prologue's vmaskf and len32 above are per pair and are replaced by the encoders' own rows, which the backward reads
                st.len32 = query_lengths(bank->qmask_q.reshape({query_features.size(0), -1}));
                st.vmaskf = project_videos(P, st.vx, bank->vmask_v.reshape({st.vx.size(0) * T}), st.fv);
                std::tie(bfw, bfs) = query_encoder(st.lstm, P, query_features, st.len32, maxq, H, false);
                bfv = st.fv;
                st.fs_bank = bfs; st.vi = bank->vi; st.qi = bank->qi;
                st.v_ptr = bank->v_ptr; st.v_pairs = bank->v_pairs; st.q_ptr = bank->q_ptr; st.q_pairs = bank->q_pairs;
            }
            // both encoders ran once per video and per query: the pairs' f = f_v * f_s, f_w and f_s in one launch (csrc/corpus.hip)
            st.fw = at::empty({Bq, maxq, (int64_t)D}, opt); st.fs = at::empty({Bq, (int64_t)D}, opt);
            if (bank->storage)
                SMIN_CK(smin_pair_assemble_compact(cur(), bfv.const_data_ptr(), bank->fv_scale.defined() ? fp(bank->fv_scale) : nullptr, bank->storage, fp(bfs), fp(bfw),
                                                   ip(bank->vi), ip(bank->qi), B, i32(bfv.size(0)), i32(bfs.size(0)), Ti, Nq, D, fpm(st.f), fpm(st.fw), fpm(st.fs)));
            else
                SMIN_CK(smin_pair_assemble(cur(), fp(bfv), fp(bfs), fp(bfw), ip(bank->vi), ip(bank->qi), B, i32(bfv.size(0)), i32(bfs.size(0)), Ti, Nq, D, fpm(st.f),
                                           fpm(st.fw), fpm(st.fs)));
        } else {
            std::tie(st.fw, st.fs) = query_encoder(st.lstm, P, query_features, st.len32, maxq, H, scoring);
            if (projection_ready) {
                await(curs, projection_ready);
                SMIN_CK(smin_video_encoder_gate(cur(), fp(st.fv), fp(st.fs), B, Ti, D, fpm(st.f)));
            } else {
                SMIN_CK(smin_video_encoder_fwd(cur(), fp(st.vx), fp(P.backbone(P_VE_W)), fp(P.backbone(P_VE_B)), fp(P.backbone(P_PE)), fp(st.vmaskf), fp(st.fs), B, Ti,
                                               i32(st.vx.size(2)), D, fpm(st.fv), fpm(st.f)));
            }
        }
    }

    // ---- layout, part 2: the one host wait (unless the caller knows the count), then the cell list on the second stream
    void layout()
    {
        if (n_known < 0) host_wait(count_ready);
        N = n_known < 0 ? host_n.const_data_ptr<int64_t>()[0] : n_known;
        n = i32(N);
        mask8 = mm.contiguous().view(at::kByte);
        if (prep != curs) await(prep, count_ready);                               // (the mask; the second stream is idle while the LSTM runs)
        StreamScope sc(prep);
        auto io = at::TensorOptions().dtype(at::kInt).device(dev);
        st.cells = at::empty({N, 4}, io); st.row_ptr = at::empty({Bq * L + 1}, io); st.cellmap = at::empty({Bq, L, L}, io);
        if (n_known < 0)
            SMIN_CK(smin_build_cells(cur(), u8(mask8), B, Li, 0, st.cells.data_ptr<int32_t>(), st.row_ptr.data_ptr<int32_t>(), st.cellmap.data_ptr<int32_t>()));
        else
            SMIN_CK(smin_build_cells_n(cur(), u8(mask8), B, Li, 0, n, st.cells.data_ptr<int32_t>(), st.row_ptr.data_ptr<int32_t>(), st.cellmap.data_ptr<int32_t>(),
                                       layout_status(dev).data_ptr<int32_t>()));
        layout_ready = mark(prep);
    }

    // ---- word-side operands on the second stream, behind the backbone; the main stream needs them at the first attention only
    void word_operands()
    {
        wait_stream(prep, curs);
        StreamScope sc(prep);
        std::vector<const float*> pp;
        for (int64_t k = 0; k < nl; ++k)
            for (int which : L_WORD_SIDE) pp.push_back(fp(P.layer(k, which)));
        st.what = at::empty({nl, B, Nq, dl}, opt); st.kb = at::empty({nl, B, Nq, dl}, opt); st.Mq = at::empty({nl, B, Nq, dl}, opt);
        st.shat = at::empty({nl, B, dl}, opt); st.uq = at::empty({nl, B, Nq}, opt);
        SMIN_CK(smin_word_prep_fwd(cur(), fp(st.fw), fp(st.fs), fp(st.qmf), pp.data(), i32(nl), B, Nq, D, dl, fpm(st.what), fpm(st.shat), fpm(st.kb), fpm(st.Mq), fpm(st.uq)));
        words_ready = mark(prep);
    }

    // ---- proposal map (f_m, f_b) and every layer's clip-window term of chat, behind the parameter products and the layout
    void proposal_map()
    {
        if (prep != curs) { await(curs, products_ready); await(curs, layout_ready); }
        fm = at::empty({N, D}, opt); fb = at::empty({B, L, D}, opt);
        {
            auto ws = SMIN_WS(smin_proposal_map_fwd_ws_bytes(B, Ti, D), dev);
            SMIN_CK(smin_proposal_map_fwd(cur(), fp(st.f), ip(st.cells), n, B, Ti, Li, Ci, D, nullptr, fpm(fm), fpm(fb), ws.p, ws.n));
        }
        pgs = at::empty({nl, N * C, dl}, opt);
        {
            Tensor g_all = at::empty({(int64_t)B * T, nl * dl}, opt);
            const Tensor* xs[1] = {&st.f};
            linear_rows_fwd(xs, 1, fp(st.Wch_all), nullptr, nullptr, nullptr, 1, i32(B * T), i32(nl * dl), D, fpm(g_all));
            auto ws = SMIN_WS(smin_clip_window_means_fwd_ws_bytes(B, Ti, dl, i32(nl)), dev);
            SMIN_CK(smin_clip_window_means_fwd(cur(), fp(g_all), fp(st.layer[0].consts), dl, ip(st.cells), n, B, Ti, Li, Ci, dl, i32(nl), fpm(pgs), ws.p, ws.n));
        }
        cumean = fm;                                                               // mean_c f_c of the proposal map is f_m
        TORCH_CHECK(!(scoring && keep_maps), "smin_score keeps no attention maps");
    }

    // ---- layer k.  The gate: hbar_k, and the later layers' running sum out of the same pass
    void gate(int64_t k)
    {
        LayerState& ls = st.layer[k];
        const bool lastl = k == nl - 1;
        ls.fm = fm; ls.fb = fb;
        ls.hbar = at::empty_like(fm);
        ls.Hs = Hs;                                                                // sum of the earlier layers' gated features (undefined for k = 0)
        if (k > 0 && !lastl && N > 0) {                                            // the next layers' running sum comes out of the same pass
            Tensor Hs_next = at::empty_like(fm);
            SMIN_CK(smin_gate_fwd_sum(cur(), fp(fm), fp(st.fs), ip(st.cells), n, D, fpm(ls.hbar), fp(Hs), fpm(Hs_next)));
            Hs = Hs_next;
        } else {
            SMIN_CK(smin_gate_fwd(cur(), fp(fm), fp(st.fs), ip(st.cells), n, D, fpm(ls.hbar)));
            if (!lastl) Hs = Hs.defined() ? Hs + ls.hbar : ls.hbar;
        }
    }

    // boundary unit on the second stream beside the content stream; joins before the moment unit (or the scoring tail)
    void boundary_unit(int64_t k)
    {
        LayerState& ls = st.layer[k];
        Tensor bmap = keep_maps ? at::empty({B, L, Nq}, opt) : Tensor();           // (allocated on the main stream, written on the boundary stream)
        wait_stream(side, curs);
        {
            StreamScope sc(side);
            ls.bu = at::empty_like(fb); ls.Qb = at::empty_like(fb); ls.baq = at::empty_like(fb); ls.bqv = at::empty_like(fb); ls.Kb = at::empty_like(st.fw);
            ls.P = at::empty({B, L, Nq}, opt); ls.A = at::empty({B, L, L}, opt);
            SMIN_CK(smin_boundary_unit_fwd(cur(), fp(fb), fp(st.fw), fp(st.fs), fp(ls.hbar), ip(st.cells), ip(st.row_ptr), n, B, Li, Nq, D, fp(P.layer(k, L_BQ_W)),
                                           fp(P.layer(k, L_BQ_B)), fp(P.layer(k, L_BK_W)), fp(P.layer(k, L_BK_B)), fp(st.qmf), fp(st.lmf), fpm(ls.bu), fpm(ls.Qb), fpm(ls.Kb),
                                           fpm(ls.P), fpm(ls.baq), fpm(ls.bqv), fpm(ls.A)));
            if (keep_maps)                                                         // Attention.attn_weights (models.py:153) is P as written
                TORCH_CHECK(hipMemcpyAsync(bmap.data_ptr(), ls.P.const_data_ptr(), sizeof(float) * ls.P.numel(), hipMemcpyDeviceToDevice, side.stream()) == hipSuccess,
                            "hipMemcpyAsync failed");
        }
        if (keep_maps) st.bmaps.push_back(bmap);
    }

    // chat_k = clip-window term + [cc_0 | ..] Pcat^T + const_k + (Hs Wch^T per cell)
    void chat(int64_t k)
    {
        LayerState& ls = st.layer[k];
        Tensor chat = pgs[k];
        for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
            Tensor hp;
            if (lo == 0) {
                hp = at::empty({N, dl}, opt);
                const Tensor* xs[1] = {&ls.Hs};
                linear_rows_fwd(xs, 1, fp(P.layer(k, L_CH_W)), nullptr, nullptr, nullptr, 1, n, dl, D, fpm(hp));
            }
            const int nseg = i32(std::min<int64_t>(4, k - lo));
            Tensor y = at::empty({N * C, dl}, opt);
            const Tensor* xs[4];
            for (int sgm = 0; sgm < nseg; ++sgm) xs[sgm] = &st.layer[lo + sgm].cc;
            linear_rows_fwd(xs, nseg, fp(ls.Pcat[part]), lo == 0 ? fp(ls.consts) : nullptr, fp(chat), fp(hp), Ci, i32(N * C), dl, dl, fpm(y));
            chat = y;
        }
        ls.chat = chat;
    }

    // the content-attention core: the first reader of the word-side operands
    void attention(int64_t k)
    {
        LayerState& ls = st.layer[k];
        const bool lastl = k == nl - 1;
        if (k == 0 && prep != curs) await(curs, words_ready);
        ls.cc = at::empty({lastl ? 0 : N * C, dl}, cc_bf16 ? opt.dtype(at::kBFloat16) : opt); ls.ccmean = at::empty({N, dl}, opt);
        Tensor probs = keep_maps ? at::empty({N * C, (int64_t)Nq}, opt) : Tensor();
        content_attn_fwd(fp(ls.chat), ip(st.cells), ip(st.row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]), fp(st.shat[k]), fp(st.qmf),
                         lastl ? Tensor() : ls.cc, fpm(ls.ccmean), probs);
        if (!keep_maps) return;
        if (flags & F_ATTN_PACKED) {
            st.cmaps.push_back(probs);
        } else {                                                                   // ContentAttention.attn_weights in the reference's layout
            Tensor dense = at::empty({Bq, L, L, C, (int64_t)Nq}, opt);
            SMIN_CK(smin_content_attn_maps_dense(cur(), fp(probs), ip(st.cellmap), ip(st.cells), B, Li, Ci, dl, Nq, fp(st.uq[k]), fp(st.qmf), fpm(dense)));
            st.cmaps.push_back(dense);
        }
    }

    // Forward only, in place of the last layer's second half: nobody but the score head reads the last mu, so the content-stream sum,
    // the moment unit and the head collapse to row dots (csrc/score_tail.hip): no cum, no x1, no mu
    void score_tail(int64_t k)
    {
        LayerState& ls = st.layer[k];
        wait_stream(curs, side);
        st.pm = at::empty({B, L, L}, opt); st.psea = at::empty({3, B, L}, opt);
        // (its vectors were formed with the parameter products; hbar is re-formed from fm and fs: measured faster than read)
        SMIN_CK(smin_score_tail_fwd(cur(), fp(ls.ccmean), fp(cumean), nullptr, fp(fm), fp(st.fs), fp(ls.bu), ip(st.cells), n, B, Li, D, dl, nullptr, nullptr, nullptr,
                                    nullptr, fp(P.loc(0)), nullptr, fp(st.wb), fp(bb), fp(st.lmf), fpm(st.pm), fpm(st.psea), st.tailv.data_ptr(),
                                    (size_t)st.tailv.numel()));
    }

    // clip-mean update: cum = ccmean Wc^T + b + cumean + hbar
    void clip_mean(int64_t k)
    {
        LayerState& ls = st.layer[k];
        ls.cum = at::empty({N, D}, opt);
        const Tensor* xs[1] = {&ls.ccmean};
        linear_rows_fwd(xs, 1, fp(P.layer(k, L_C_W)), fp(P.layer(k, L_C_B)), fp(cumean), fp(ls.hbar), 1, n, D, dl, fpm(ls.cum));
    }

    // The moment unit, behind the boundary unit; its outputs are the next layer's inputs.  The pair product f_b[i] * f_b[j] is kept for
    // the weight gradient (bf16 under bf16_operands: the layer's largest saved tensor); a scorer has no use for it and lets the
    // contraction form the product as it loads (measured faster there)
    void moment_unit(int64_t k)
    {
        LayerState& ls = st.layer[k];
        wait_stream(curs, side);
        Tensor mu = at::empty_like(fm);
        if (!scoring) ls.x1 = bf16_operands ? at::empty({N, D}, opt.dtype(at::kBFloat16)) : at::empty_like(fm);
        moment_unit_fwd(fp(ls.cum), fp(fm), fp(ls.bu), ip(st.cells), n, B, Li, D, fp(ls.Wcat), fp(bcat[k]), fpm(mu), ls.x1);
        fm = mu; cumean = ls.cum; fb = ls.bu;
    }

    // Localization (models.py:335-344)
    void score_head()
    {
        Tensor pm = at::empty({B, L, L}, opt), psea = at::empty({3, B, L}, opt);
        SMIN_CK(smin_score_map_fwd(cur(), fp(fm), fp(fb), ip(st.cells), n, B, Li, D, fp(P.loc(0)), fp(P.loc(1)), fp(st.wb), fp(bb), fp(st.lmf), fpm(pm), fpm(psea)));
        st.pm = pm; st.psea = psea; st.fm_out = fm;
    }
};

}  // namespace
