// The backward pass of the one-node core as a schedule of stages (SminCore::backward lists them in order).
#pragma once
#include "core_state.h"

namespace {

// What one layer's stages hand to each other; gone when the layer is done (dcum and dfb_k live on as dcum_next / dfb_next)
struct LayerGrads { Tensor dcum, dfb_mu, dfb_k, dbu, dccmean, dhp; };

// The backward pass of the state the forward left: the parameters' gradients in slots N_FIXED .. of the result, the inputs'
// (F_INPUT_GRADS) in slots 0 and 1.  With the pair lists in the state (smin_forward_pairs) everything down to
// df, dfs_parts and dfw_parts runs at batch P as it stands; smin_pair_assemble_bwd then sums the pairs onto their videos and
// queries, and the backbone's backward runs at batch V (video encoder) and Q (sentence feature, LSTM layers).
// Streams: the caller's (`curs`), the boundary unit's (`side`), the weight gradients' (`wstr`), and in the tail `tail`, `wordst`, `cw`
// and `bstr`, each of which is one of the former or the second side stream.  The members are what outlives a stage: the gradient
// accumulators, the events of hand-offs that cross stages, and every tensor another stream reads until the streams join -- those
// that no member holds by name are in `keep` ("Stream rules" (2) and (4)).
struct BackwardPass : Dims {
    AutogradContext* const ctx;
    const variable_list& g;
    CoreState& st;
    const ParamList& P;
    const int64_t N, T, L, C, nl, flags, H, Nq_in;
    const Tensor &f, &fw, &fs, &qmf, &lmf, &cells, &row_ptr, &cellmap;
    const int n;
    const bool prep_kernel;
    ParamList dprm;                                             // the gradients, slot for slot
    // weight-gradient contractions: nothing waits for them before the end of the step, so they go to a low-priority stream
    // of their own and fill the chip beside the bandwidth-bound kernels of the main chain
    const HStream wstr;
    // (the transposes and the boundary heads' backward on the boundary stream: beside the score map's backward on the main stream, which
    //  otherwise opens the backward pass with four short launches in a row in front of the first contraction)
    const HStream early;
    std::vector<Tensor> keep;                                   // main-stream tensors read on other streams: alive until the streams join
    GradSync sync;
    // the inputs' gradients (F_INPUT_GRADS): d video_features = the video encoder's dx, d query_features = LSTM layer 0's dX
    const bool want_dx, want_dX;
    // W^T of every contraction weight: TR_PER_LAYER per layer, every layer's Pcat parts (PcatT), then from tr_tail on Wch_all, the two
    // LSTM layers' Wih and, for want_dx, the video encoder's W
    enum { TR_CH = 0, TR_C, TR_CAT, TR_BQ, TR_BK, TR_PER_LAYER };
    std::vector<Tensor> tr;
    std::vector<std::vector<Tensor>> PcatT, dPcat;
    size_t tr_tail = 0;
    Tensor dpm, dpsea, dfm, dfb_next;                           // the scores' gradients; the running gradients of f_m and f_b
    Tensor dcum_next;                                           // gradient of cum_k from layer k+1's clip-mean chain
    std::vector<Tensor> loc_bufs, lstm_bufs, dcc, dHs, dchat, dconsts, dfs_parts, dfw_parts, base_ch, base_c, base_bc;
    // prep_kernel: the gradients that meet in the parameter products are gathered as the kernel of csrc/param_prep.hip wants them
    Tensor dconsts_all, dWcat_all, dbcat_all, dWch_all, dwhat, dshat, dMq, duq;
    hipEvent_t attn0_done = nullptr, words_done = nullptr, weights_done = nullptr;
    hipEvent_t boundary_done = nullptr;                         // the previous layer's boundary-unit backward (side stream)
    bool tail_split = false;
    HStream tail, wordst, cw, bstr;                             // the tail's streams (tail_streams)
    // the backbone: the rows of the video encoder and of the query encoder (B unless pairs), and what its stages hand to each other
    const bool pairs;
    const int Din, Bv, Bw;
    Tensor df, wsv, dfs_video, dfs_total, dfw_total, venc_fs, dH, dvideo, dquery;

    BackwardPass(AutogradContext* ctx, const variable_list& g, const SavedShape& s, CoreState& st, const ParamList& P)
        : Dims(st.f, st.f.size(0), P, s.T, s.L, s.C, st.fw.size(1), s.flags), ctx(ctx), g(g), st(st), P(P), N(s.N), T(s.T), L(s.L), C(s.C), nl(s.nl), flags(s.flags), H(s.H),
          Nq_in(s.Nq_in), f(st.f), fw(st.fw), fs(st.fs), qmf(st.qmf), lmf(st.lmf), cells(st.cells), row_ptr(st.row_ptr), cellmap(st.cellmap), n(i32(N)),
          prep_kernel((flags & F_PARAM_PREP_KERNEL) != 0), dprm(nl), wstr((flags & F_ASYNC_WEIGHTS) ? weight_stream(dev.index()) : curs),
          early((side != curs && (flags & F_OVERLAP_PREP)) ? side : curs), want_dx((flags & F_INPUT_GRADS) && ctx->needs_input_grad(0)),
          want_dX((flags & F_INPUT_GRADS) && ctx->needs_input_grad(1)), PcatT(nl), dPcat(nl), dcc(nl), dHs(nl), dchat(nl), dconsts(nl), base_ch(nl), base_c(nl), base_bc(nl),
          tail(curs), wordst(curs), cw(curs), bstr(curs), pairs(st.vi.defined()), Din(i32(st.vx.size(2))), Bv(i32(st.vx.size(0))), Bw(i32(st.lstm[0].x.size(0)))
    {
        sync.on = (flags & F_GRAD_SYNC) != 0;
        TORCH_CHECK(!sync.on || prep_kernel, "smin_forward: the in-node gradient exchange needs param_prep_kernel (SMIN._param_prep_kernel)");
        TORCH_CHECK(!sync.on || !grad_sync_config().group.empty(), "smin_forward: grad_sync requested but no process group was set (smin_hip::set_grad_sync)");
    }
    static void acc(Tensor& into, const Tensor& t) { if (into.defined()) into.add_(t); else into = t; }
    const Tensor& trk(int64_t k, int which) const { return tr[k * TR_PER_LAYER + which]; }

    // ---- W^T of every contraction weight, one launch
    void transposes()
    {
        std::vector<Tensor> tr_in;
        for (int64_t k = 0; k < nl; ++k) {
            for (const Tensor& w : {P.layer(k, L_CH_W), P.layer(k, L_C_W), st.layer[k].Wcat, P.layer(k, L_BQ_W), P.layer(k, L_BK_W)}) tr_in.push_back(w);
        }
        const size_t tr_pcat0 = tr_in.size();
        for (int64_t k = 0; k < nl; ++k) for (auto& p : st.layer[k].Pcat) tr_in.push_back(p);
        tr_tail = tr_in.size();
        tr_in.push_back(st.Wch_all);
        tr_in.push_back(st.lstm[0].Wih); tr_in.push_back(st.lstm[1].Wih);
        if (want_dx) tr_in.push_back(P.backbone(P_VE_W));
        wait_stream(early, curs);
        {
            StreamScope sc(early);
            tr = transpose_all(tr_in);
        }
        { size_t i = tr_pcat0; for (int64_t k = 0; k < nl; ++k) for (size_t p = 0; p < st.layer[k].Pcat.size(); ++p) PcatT[k].push_back(tr[i++]); }
    }

    // ---- Localization: the score map's backward; with a second stream the boundary heads' half runs there, beside the moment map's
    void localization_head()
    {
        const Tensor& bu_last = st.layer[nl - 1].bu;
        dpm = g[0].defined() ? cont(g[0]) : at::zeros_like(st.pm);
        {
            // the three score gradients as one (3, B, L) buffer: the library's loss hands over rows of one buffer (used as it is);
            // anything else is gathered
            const int64_t BL = (int64_t)B * L;
            bool rows = g[1].defined() && g[2].defined() && g[3].defined();
            for (int h = 1; rows && h <= 3; ++h) rows = g[h].scalar_type() == at::kFloat && g[h].is_contiguous() && g[h].numel() == BL;
            if (rows && fp(g[2]) == fp(g[1]) + BL && fp(g[3]) == fp(g[1]) + 2 * BL) dpsea = g[1];
            else {
                std::vector<Tensor> parts;
                for (int h = 1; h <= 3; ++h) parts.push_back(g[h].defined() ? fl(g[h]).reshape({B, L}) : at::zeros({B, L}, opt));
                dpsea = at::stack(parts);
            }
        }
        dfm = at::empty({N, D}, opt); dfb_next = at::empty({B, L, D}, opt);
        Tensor dwm = at::empty({D}, opt), dbm = at::empty({1}, opt), dwb = at::empty({3, D}, opt), dbb = at::empty({3}, opt);
        if (early != curs) {
            wait_stream(early, curs);                                              // (behind the allocations above: "Stream rules" (2))
            {
                StreamScope sc(early);
                auto ws = SMIN_WS(smin_score_map_bwd_ws_bytes(n, B, Li, D), dev);
                SMIN_CK(smin_score_map_bwd(cur(), nullptr, fp(dpsea), fp(st.pm), fp(st.psea), fp(st.fm_out), fp(bu_last), ip(cells), n, B, Li, D, fp(P.loc(0)), fp(st.wb),
                                           fp(lmf), nullptr, fpm(dfb_next), nullptr, nullptr, fpm(dwb), fpm(dbb), ws.p, ws.n));
            }
            hipEvent_t early_done = mark(early);
            auto ws = SMIN_WS(smin_score_map_bwd_ws_bytes(n, B, Li, D), dev);
            SMIN_CK(smin_score_map_bwd(cur(), fp(dpm), nullptr, fp(st.pm), fp(st.psea), fp(st.fm_out), fp(bu_last), ip(cells), n, B, Li, D, fp(P.loc(0)), fp(st.wb), fp(lmf),
                                       fpm(dfm), nullptr, fpm(dwm), fpm(dbm), nullptr, nullptr, ws.p, ws.n));
            await(curs, early_done);                                               // W^T and dfb_next
        } else {
            auto ws = SMIN_WS(smin_score_map_bwd_ws_bytes(n, B, Li, D), dev);
            SMIN_CK(smin_score_map_bwd(cur(), fp(dpm), fp(dpsea), fp(st.pm), fp(st.psea), fp(st.fm_out), fp(bu_last), ip(cells), n, B, Li, D, fp(P.loc(0)), fp(st.wb), fp(lmf),
                                       fpm(dfm), fpm(dfb_next), fpm(dwm), fpm(dbm), fpm(dwb), fpm(dbb), ws.p, ws.n));
        }
        loc_bufs = {dwm, dbm, dwb, dbb};
        dprm.loc(0) = dwm.view_as(P.loc(0)); dprm.loc(1) = dbm.view_as(P.loc(1));
        for (int h = 0; h < 3; ++h) { dprm.loc(2 + 2 * h) = dwb[h].view_as(P.loc(2 + 2 * h)); dprm.loc(3 + 2 * h) = dbb.slice(0, h, h + 1).view_as(P.loc(3 + 2 * h)); }
    }

    // the accumulators the layers write into: the parameter products' inputs and the word-side operands' gradients
    void accumulators()
    {
        if (prep_kernel) {
            dconsts_all = at::empty({nl, dl}, opt); dWcat_all = at::empty({nl, D, 2 * D}, opt); dbcat_all = at::empty({nl, D}, opt);
            for (int64_t k = 0; k < nl; ++k) dconsts[k] = dconsts_all[k];
        }
        dwhat = at::empty_like(st.what); dshat = at::empty_like(st.shat); dMq = at::empty_like(st.Mq); duq = at::empty_like(st.uq);
        if (N == 0) { dwhat.zero_(); dshat.zero_(); dMq.zero_(); duq.zero_(); }
    }

    // ---- layer k, descending
    void layer(int64_t k)
    {
        LayerGrads lg;
        moment_unit_weights(k, lg);
        moment_unit_inputs(k, lg);
        boundary_unit(k, lg);
        clip_mean(k, lg);
        attention(k, lg);
        chat_inputs(k, lg);
        content_weights(k, lg);
        gate(k, lg);
        dcum_next = lg.dcum; dfb_next = lg.dfb_k;
    }

    // moment unit: dmu -> d cum (its chain gradient folded in), d bu, weight gradients; the residual gradient is dmu itself.
    // The weight half on the weight stream, queued ahead of the input half (measured: 21.39 -> 21.15 ms/step, behind it 21.7 -> 21.6)
    void moment_unit_weights(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        lg.dcum = at::empty({N, D}, opt); lg.dfb_mu = at::empty({B, L, D}, opt);
        keep.push_back(dfm); keep.push_back(lg.dcum);
        wait_stream(wstr, curs);
        StreamScope sc(wstr);
        Tensor dWcat = prep_kernel ? dWcat_all[k] : at::empty_like(ls.Wcat), dbcat = prep_kernel ? dbcat_all[k] : at::empty({D}, opt);
        auto ws = SMIN_WS(smin_moment_unit_bwd_ws_bytes(n, B, Li, D), dev);
        moment_unit_bwd(fp(dfm), fp(ls.cum), fp(ls.bu), ip(cells), ip(row_ptr), ip(cellmap), n, B, Li, D, fp(trk(k, TR_CAT)), nullptr, nullptr, fpm(dWcat), fpm(dbcat), ws,
                        nullptr, ls.x1, nullptr);
        if (!prep_kernel) {
            dprm.layer(k, L_FB_W) = dWcat.slice(1, 0, D).contiguous().view_as(P.layer(k, L_FB_W));
            dprm.layer(k, L_FC_W) = dWcat.slice(1, D).contiguous().view_as(P.layer(k, L_FC_W));
            dprm.layer(k, L_FB_B) = dbcat; dprm.layer(k, L_FC_B) = dbcat;
        }
        sync.reduce({dWcat, dbcat}, wstr);                                           // inputs of the parameter-product kernel
    }

    // The input half.  The previous layer's boundary-unit backward (second stream) is awaited HERE, where its dfb is first read -- not in
    // front of that layer's gate backward, which reads nothing of it any more (it forms the unit's dhbar itself): the main stream sat
    // ~0.6 ms behind the unit's weight contractions at the end of layer 0 (tools/gantt.sh)
    void moment_unit_inputs(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        if (boundary_done) { await(curs, boundary_done); boundary_done = nullptr; }
        auto ws = SMIN_WS(smin_moment_unit_bwd_ws_bytes(n, B, Li, D), dev);
        moment_unit_bwd(fp(dfm), fp(ls.cum), fp(ls.bu), ip(cells), ip(row_ptr), ip(cellmap), n, B, Li, D, fp(trk(k, TR_CAT)), fpm(lg.dcum), fpm(lg.dfb_mu), nullptr, nullptr, ws,
                        fp(dcum_next), Tensor(), fp(dfb_next));                    // (the pair product feeds the weight half only)
    }                                                                              // dfb_mu = this unit's gradient of bu + the later consumer's (dfb_next): dbu

    // boundary unit on the second stream
    // (the boundary unit's gradient of hbar, A[b,i,j] * dbu[b,i,:], is formed by the gate backward itself from A and dbu: no [N][D]
    //  tensor written here and read back there)
    void boundary_unit(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        wait_stream(side, curs);
        {
            StreamScope sc(side);
            lg.dbu = lg.dfb_mu;
            lg.dfb_k = at::empty({B, L, D}, opt);
            Tensor dfw = at::empty_like(fw), dfs = at::empty_like(fs);
            Tensor dWq = at::empty({D, D}, opt), dbq = at::empty({D}, opt), dWk = at::empty({D, D}, opt), dbk = at::empty({D}, opt);
            auto ws = SMIN_WS(smin_boundary_unit_bwd_ws_bytes(B, Li, Nq, D), dev);
            SMIN_CK(smin_boundary_unit_bwd(cur(), fp(lg.dbu), fp(ls.fb), fp(fw), fp(fs), fp(ls.hbar), ip(cells), ip(row_ptr), n, B, Li, Nq, D, fp(trk(k, TR_BQ)),
                                           fp(trk(k, TR_BK)), fp(qmf), fp(lmf), fp(ls.Qb), fp(ls.Kb), fp(ls.P), fp(ls.baq), fp(ls.bqv), fp(ls.A), fpm(lg.dfb_k), fpm(dfw), fpm(dfs),
                                           nullptr, fpm(dWq), fpm(dbq), fpm(dWk), fpm(dbk), ws.p, ws.n));
            dprm.layer(k, L_BQ_W) = dWq; dprm.layer(k, L_BQ_B) = dbq; dprm.layer(k, L_BK_W) = dWk; dprm.layer(k, L_BK_B) = dbk;
            sync.reduce({dWq, dbq, dWk, dbk}, side);
            dfs_parts.push_back(dfs); dfw_parts.push_back(dfw);
            keep.push_back(dfb_next); keep.push_back(lg.dfb_mu); keep.push_back(lg.dbu);
        }
        if (side != curs) boundary_done = mark(side);
    }

    // clip-mean update cum = ccmean Wc^T + b + cumean + hbar: d ccmean (the weight gradients: content_weights); d cumean = d hbar = dcum
    void clip_mean(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        lg.dccmean = at::empty({N, dl}, opt);
        const float* xs[1] = {fp(ls.ccmean)}; float* dxs[1] = {fpm(lg.dccmean)};
        auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, D, dl), dev);
        SMIN_CK(smin_linear_rows_bwd(cur(), fp(lg.dcum), xs, 1, fp(trk(k, TR_C)), n, D, dl, dxs, nullptr, nullptr, ws.p, ws.n));
    }

    // attention core
    void attention(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        dchat[k] = at::empty({N * C, dl}, opt);
        if (N > 0) {
            auto ws = scratch(smin_content_attn_bwd_workspace_bytes(n, B, Ci, dl), dev);
            SMIN_CK(smin_content_attn_bwd(cur(), fp(dcc[k]), fp(lg.dccmean), fp(ls.chat), ip(cells), ip(row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]),
                                          fp(st.shat[k]), fp(qmf), fpm(dchat[k]), fpm(dMq[k]), fpm(duq[k]), fpm(dwhat[k]), fpm(dshat[k]), ws.p, ws.n));
        }
        if (k == 0) attn0_done = mark(curs);                                    // every dchat / word-side gradient is final from here on
    }

    // chat_k's contraction over the earlier layers' attention outputs, and its per-cell gate term: input gradients
    void chat_inputs(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
            const int nseg = i32(std::min<int64_t>(4, k - lo));
            const float* xs[4]; float* dxs[4];
            // every earlier layer's attention output already has the gradient of the later layers (all of them, or none for the last
            // layer): accumulate in the epilogue instead of a full-size add per tensor afterwards
            const bool have = dcc[lo].defined();
            for (int sgm = 0; sgm < nseg; ++sgm) {
                TORCH_CHECK(dcc[lo + sgm].defined() == have, "content stream: inconsistent gradient state of the attention outputs");
                xs[sgm] = nullptr;                                                 // (the input gradients never read the operands)
                if (!have) dcc[lo + sgm] = at::empty({N * C, dl}, opt);
                dxs[sgm] = fpm(dcc[lo + sgm]);
            }
            if (have) {
                SMIN_CK(smin_linear_rows_dx_acc(cur(), fp(dchat[k]), nseg, fp(PcatT[k][part]), i32(N * C), dl, dl, dxs));
            } else {
                auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(i32(N * C), dl, nseg * dl), dev);
                SMIN_CK(smin_linear_rows_bwd(cur(), fp(dchat[k]), xs, nseg, fp(PcatT[k][part]), i32(N * C), dl, dl, dxs, nullptr, nullptr, ws.p, ws.n));
            }
        }
        if (k > 0) {
            lg.dhp = at::empty({N, dl}, opt);
            keep.push_back(lg.dhp);
            SMIN_CK(smin_group_sum(cur(), fp(dchat[k]), n, Ci, dl, fpm(lg.dhp)));
            dHs[k] = at::empty({N, D}, opt);
            const float* xs[1] = {fp(ls.Hs)}; float* dxs[1] = {fpm(dHs[k])};
            auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, dl, D), dev);
            SMIN_CK(smin_linear_rows_bwd(cur(), fp(lg.dhp), xs, 1, fp(trk(k, TR_CH)), n, dl, D, dxs, nullptr, nullptr, ws.p, ws.n));
        }
    }

    // ... and this layer's weight gradients of the content stream, on the weight stream
    void content_weights(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        wait_stream(wstr, curs);
        StreamScope sc(wstr);
        {
            Tensor dWc = at::empty_like(P.layer(k, L_C_W)), dbc = at::empty({D}, opt);
            const Tensor* xs[1] = {&ls.ccmean};
            auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, D, dl), dev);
            linear_rows_bwd_weights(fp(lg.dcum), xs, 1, n, D, dl, fpm(dWc), fpm(dbc), ws);
            if (prep_kernel) { base_c[k] = dWc; base_bc[k] = dbc; }
            else { acc(dprm.layer(k, L_C_W), dWc); acc(dprm.layer(k, L_C_B), dbc); }
        }
        for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
            const int nseg = i32(std::min<int64_t>(4, k - lo));
            Tensor dP = at::empty_like(ls.Pcat[part]);
            if (lo == 0 && !prep_kernel) dconsts[k] = at::empty({dl}, opt);
            auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(i32(N * C), dl, nseg * dl), dev);
            const Tensor* xs[4];
            for (int sgm = 0; sgm < nseg; ++sgm) xs[sgm] = &st.layer[lo + sgm].cc;
            linear_rows_bwd_weights(fp(dchat[k]), xs, nseg, i32(N * C), dl, dl, fpm(dP), lo == 0 ? fpm(dconsts[k]) : nullptr, ws);
            dPcat[k].push_back(dP);
        }
        if (k > 0) {
            Tensor dWch = at::empty_like(P.layer(k, L_CH_W));
            const Tensor* xs[1] = {&ls.Hs};
            auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, dl, D), dev);
            linear_rows_bwd_weights(fp(lg.dhp), xs, 1, n, dl, D, fpm(dWch), nullptr, ws);
            if (prep_kernel) base_ch[k] = dWch; else acc(dprm.layer(k, L_CH_W), dWch);
        }
    }

    // gate: every consumer of hbar_k (clip-mean update, boundary unit, the later layers' running sums) and of f_m (residual; layer 0: the clip-mean chain)
    void gate(int64_t k, LayerGrads& lg)
    {
        LayerState& ls = st.layer[k];
        std::vector<Tensor> later;
        for (int64_t kk = k + 1; kk < nl; ++kk) later.push_back(dHs[kk]);
        std::vector<const float*> dh{fp(lg.dcum)}, dr{fp(dfm)};
        Tensor later_sum;
        if (later.size() <= 3) for (auto& t : later) dh.push_back(fp(t));
        else { later_sum = sum_list(later); dh.push_back(fp(later_sum)); }
        if (k == 0) dr.push_back(fp(lg.dcum));
        Tensor dfm_k = at::empty({N, D}, opt), dfs = at::empty_like(fs);
        auto ws = SMIN_WS(smin_gate_bwd_ws_bytes(B, Li, D), dev);
        SMIN_CK(smin_gate_bwd(cur(), dh.data(), i32(dh.size()), dr.data(), i32(dr.size()), fp(ls.fm), fp(fs), ip(row_ptr), n, B, Li, D, fpm(dfm_k), fpm(dfs), ws.p, ws.n,
                              ip(cells), fp(ls.A), fp(lg.dbu)));
        dfs_parts.push_back(dfs);
        dfm = dfm_k;
    }

    // ---- the tail.  Three chains leave the last attention backward (layer 0's) and meet again in front of the LSTM layers:
    //   words  (own stream): the word-side operands' backward, 0.75 ms of small-grid kernels at ActivityNet size -> d f_w
    //   tail   (the boundary stream): the clip-window gradients of every layer's chat -> dg; later the parameter products
    //   main   : layer 0's gate backward (already queued above), the proposal map's gradient -> df, video encoder, LSTM layers
    // (before: the first two waited for the gate backward and the clip-window pass sat between it and the proposal map on the
    //  main stream -- 0.5 ms longer, tools/gantt.sh)
    // Without F_TAIL_SPLIT: the round-2 placement (words on the boundary stream, clip-window gradients on the main stream).
    // training.CapturedStep asks for it: a replayed graph pays for the extra streams (tacos.yml captured: 3.5 ms/step once the
    // process has used them, 2.5 without; eager 2.2) -- and never inside a stream capture.
    void tail_streams()
    {
        hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
        TORCH_CHECK(hipStreamIsCapturing(curs.stream(), &capture) == hipSuccess, "hipStreamIsCapturing failed");
        tail_split = (flags & F_TAIL_SPLIT) && capture == hipStreamCaptureStatusNone;
        tail = (flags & F_OVERLAP_PREP) ? side_stream(dev.index()) : curs;
        wordst = !(flags & F_OVERLAP_PREP) ? curs : tail_split ? side_stream(dev.index(), 1) : tail;
        cw = tail_split ? tail : curs;                                              // stream of the clip-window gradients
        // the backbone's weight halves: on the word stream (idle by then) when there is one -- the weight stream still holds layer 0's
        // moment-unit contraction, and these short kernels close the step
        bstr = (tail_split && wordst != curs && wstr != curs) ? wordst : wstr;
        if (!attn0_done) attn0_done = mark(curs);
    }

    // the word-side operands' backward on the words stream, and the gradient exchange of what is final behind it
    void word_gradients()
    {
        if (!tail_split) wait_stream(wordst, curs);
        else if (wordst != curs) await(wordst, attn0_done);
        StreamScope sc(wordst);
        std::vector<const float*> gp[4], pp;
        std::vector<float*> dp;
        for (int64_t k = 0; k < nl; ++k) {
            gp[0].push_back(fp(dwhat[k])); gp[1].push_back(fp(dshat[k])); gp[2].push_back(fp(dMq[k])); gp[3].push_back(fp(duq[k]));
            for (int which : L_WORD_SIDE) {
                pp.push_back(fp(P.layer(k, which)));
                dprm.layer(k, which) = at::empty_like(P.layer(k, which));
                dp.push_back(fpm(dprm.layer(k, which)));
            }
        }
        Tensor dfw = at::empty_like(fw), dfs = at::empty_like(fs);
        auto ws = scratch(smin_word_prep_bwd_workspace_bytes(i32(nl), B, Nq, D, dl), dev);
        SMIN_CK(smin_word_prep_bwd(cur(), gp[0].data(), gp[1].data(), gp[2].data(), gp[3].data(), fp(fw), fp(fs), fp(qmf), fp(st.what), fp(st.kb), pp.data(), i32(nl), B, Nq, D,
                                   dl, fpm(dfw), fpm(dfs), dp.data(), ws.p, ws.n));
        dfw_parts.push_back(dfw); dfs_parts.push_back(dfs);
        words_done = mark(wordst);
        if (sync.on) {
            std::vector<Tensor> ws_grads = loc_bufs;
            for (int64_t k = 0; k < nl; ++k)
                for (int which : L_WORD_SIDE) ws_grads.push_back(dprm.layer(k, which));
            sync.reduce(ws_grads, wordst);
        }
    }

    // ---- clip-window terms of chat (tail stream), the proposal map (main stream), f
    void clip_windows_and_proposal_map()
    {
        bool tab_built = false;
        auto tab = clip_event_table(dev, Ti, Li, Ci, &tab_built);
        if (tab_built) wait_stream(cw, curs);                                    // first backward of this geometry only ("Stream rules" (1))
        std::vector<const float*> ptrs;
        for (int64_t k = 0; k < nl; ++k) ptrs.push_back(fp(dchat[k]));
        if (cw != curs) await(cw, attn0_done);
        hipEvent_t dg_done;
        Tensor dg;
        {
            StreamScope sc(cw);
            // allocated under THIS stream ("Stream rules" (2)): main-stream kernels are queued behind attn0_done
            dg = at::empty({(int64_t)B * T, nl * dl}, opt);
            keep.push_back(dg);
            auto ws = SMIN_WS(smin_clip_window_means_bwd_ws_bytes(B, Ti, dl, i32(nl)), dev);
            SMIN_CK(smin_clip_window_means_bwd(cur(), ptrs.data(), ip(cells), ip(row_ptr), ip(cellmap), n, B, Ti, Li, Ci, dl, i32(nl), fpm(dg), ws.p, ws.n, ip(tab.first),
                                               tab.second.data_ptr()));
            dg_done = mark(cw);
        }
        if (!tail_split) wait_stream(wstr, curs);
        {
            StreamScope sc(tail_split ? tail : wstr);
            // the weight gradient of the clip-window contraction stays on this stream (its only consumer is the parameter-product kernel
            // queued here below).  NOT on the weight stream: that stream would wait for this one and this one for it ("Stream rules" (3)).
            if (!prep_kernel) dconsts[0] = at::empty({dl}, opt);
            const Tensor* xs[1] = {&f};
            dWch_all = at::empty_like(st.Wch_all);
            auto wsw = scratch(smin_linear_rows_bwd_workspace_bytes(i32(B * T), i32(nl * dl), D), dev);
            linear_rows_bwd_weights(fp(dg), xs, 1, i32(B * T), i32(nl * dl), D, fpm(dWch_all), nullptr, wsw);
            if (!prep_kernel) for (int64_t k = 0; k < nl; ++k) acc(dprm.layer(k, L_CH_W), dWch_all.slice(0, k * dl, (k + 1) * dl));
            // layer 0's constant: its gradient is the column sum of dchat_0 (the later layers' ride on their weight-gradient passes)
            auto wsc = scratch(smin_col_sum_workspace_bytes(i32(N * C), dl), dev);
            SMIN_CK(smin_col_sum(cur(), fp(dchat[0]), i32(N * C), dl, fpm(dconsts[0]), wsc.p, wsc.n));
        }
        // df = gradient through the proposal map (f_m, f_b) + gradient through the clip-window terms, the second accumulated by its
        // contraction's epilogue
        df = at::empty({B, T, D}, opt);
        if (boundary_done) { await(curs, boundary_done); boundary_done = nullptr; }   // layer 0's dfb
        auto ws3 = SMIN_WS(smin_proposal_map_bwd_ws_bytes(B, Ti, D), dev);
        SMIN_CK(smin_proposal_map_bwd(cur(), nullptr, fp(dfm), fp(dfb_next), ip(cells), ip(row_ptr), ip(cellmap), n, B, Ti, Li, Ci, D, fpm(df), ws3.p, ws3.n, ip(tab.first),
                                      tab.second.data_ptr()));
        weights_done = mark(wstr);
        float* dxs[1] = {fpm(df)};
        if (cw != curs) await(curs, dg_done);
        SMIN_CK(smin_linear_rows_dx_acc(cur(), fp(dg), 1, fp(tr[tr_tail]), i32(B * T), i32(nl * dl), D, dxs));
    }

    // ---- the parameter products' backward on the tail stream, behind the weight stream: consts_k = b_ch_k + Wch_k bsum_k
    // (bsum_k = sum_{l<k} b_c_l), Pcat_k = [Wch_k Wc_l]_l.  With the exchange on, every input of the products is averaged first.
    void parameter_products()
    {
        if (tail != wstr) await(tail, weights_done);
        if (sync.on) {
            std::vector<Tensor> ins{dconsts_all, dWch_all};
            for (int64_t k = 0; k < nl; ++k) {
                ins.push_back(base_ch[k]); ins.push_back(base_c[k]); ins.push_back(base_bc[k]);
                for (auto& t : dPcat[k]) ins.push_back(t);
            }
            sync.reduce(ins, tail);
            sync.join(tail);                                                        // every input of the parameter products (the layers' dWcat included) is averaged
        }
        StreamScope sc(tail);
        if (prep_kernel) {
            std::vector<const float*> pp, dpc(nl * 2, nullptr), bch(nl, nullptr), bc(nl), bbc(nl);
            std::vector<float*> gp;
            for (int64_t k = 0; k < nl; ++k) {
                for (int which : L_PRODUCTS) {
                    pp.push_back(fp(P.layer(k, which)));
                    dprm.layer(k, which) = at::empty_like(P.layer(k, which));
                    gp.push_back(fpm(dprm.layer(k, which)));
                }
                for (size_t part = 0; part < dPcat[k].size(); ++part) dpc[k * 2 + part] = fp(dPcat[k][part]);
                bch[k] = fp(base_ch[k]); bc[k] = fp(base_c[k]); bbc[k] = fp(base_bc[k]);
            }
            SMIN_CK(smin_param_prep_bwd(cur(), pp.data(), i32(nl), D, dl, dpc.data(), fp(dconsts_all), fp(dWcat_all), fp(dbcat_all), fp(dWch_all), bch.data(), bc.data(),
                                        bbc.data(), gp.data()));
            return;
        }
        Tensor bsum;
        std::vector<Tensor> bsums(nl);
        for (int64_t k = 0; k < nl; ++k) { bsums[k] = bsum; bsum = bsum.defined() ? bsum + P.layer(k, L_C_B) : P.layer(k, L_C_B); }
        Tensor dbsum_run;                                                           // sum_{k' > l} Wch_k'^T dconst_k'
        for (int64_t k = nl - 1; k >= 0; --k) {
            dprm.layer(k, L_CH_B) = dconsts[k];
            if (dbsum_run.defined()) dprm.layer(k, L_C_B).add_(dbsum_run);           // in place: the buffer was allocated on the main stream and must outlive this launch
            if (k > 0) {
                dprm.layer(k, L_CH_W).addr_(dconsts[k], bsums[k]);
                Tensor dbs = at::mv(trk(k, TR_CH), dconsts[k]);
                dbsum_run = dbsum_run.defined() ? dbsum_run + dbs : dbs;
            }
            for (size_t part = 0; part < dPcat[k].size(); ++part)
                for (int64_t l = (int64_t)part * 4; l < std::min<int64_t>((int64_t)part * 4 + 4, k); ++l) {
                    Tensor dP = dPcat[k][part].slice(1, (l - (int64_t)part * 4) * dl, (l - (int64_t)part * 4 + 1) * dl);
                    dprm.layer(k, L_CH_W).addmm_(dP, trk(l, TR_C));                   // dWch_k += dP_kl Wc_l^T
                    dprm.layer(l, L_C_W).addmm_(trk(k, TR_CH), dP);                   // dWc_l  += Wch_k^T dP_kl
                }
        }
    }

    // ---- backbone on the main stream: video encoder, sentence / word features, the two LSTM layers (models.py:38-83).
    // Every call is split into its inputs half (main stream, the dependent chain) and its weights half (`bstr`); the
    // intermediate of a pair lives in a buffer of its own (the per-stream scratch is reused by the next call on that stream)
    Tensor own(size_t nbytes)
    {
        Tensor t = at::empty({(int64_t)nbytes + 256}, at::TensorOptions().dtype(at::kByte).device(dev));
        keep.push_back(t);
        return t;
    }
    void backbone_buffers()
    {
        const int64_t pe_rows = P.backbone(P_PE).size(0);
        dfs_video = at::empty({(int64_t)Bv, (int64_t)D}, opt);
        dprm.backbone(P_VE_W) = at::empty({D, Din}, opt); dprm.backbone(P_VE_B) = at::empty({D}, opt);
        dprm.backbone(P_PE) = pe_rows != T ? at::zeros({pe_rows, D}, opt) : at::empty({T, D}, opt);
        wsv = own(smin_video_encoder_bwd_workspace_bytes(Bv, Ti, Din, D));
        venc_fs = fs;
    }

    // The pairs' gradients onto their videos and queries (csrc/corpus.hip): df -> dfv, the per-pair sums of dfw / dfs and the
    // product's gradient of f_s -> the query bank's rows.  The video encoder's backward has no fs == NULL mode: it takes dfv as
    // its df and ones as fs (a multiplication by 1.0f is exact; its dfs output is not used).
    void pair_assemble()
    {
        if (wordst != curs) await(curs, words_done);
        Tensor dfs_p = sum_list(dfs_parts), dfw_p = sum_list(dfw_parts);
        Tensor dfv = at::empty_like(st.fv);
        dfw_total = at::empty({(int64_t)Bw, (int64_t)Nq, (int64_t)D}, opt); dfs_total = at::empty({(int64_t)Bw, (int64_t)D}, opt);
        Tensor wsp = own(smin_pair_assemble_bwd_workspace_bytes(B, Ti, D));
        SMIN_CK(smin_pair_assemble_bwd(cur(), fp(df), fp(dfw_p), fp(dfs_p), fp(st.fv), fp(st.fs_bank), ip(st.vi), ip(st.qi), ip(st.v_ptr), ip(st.v_pairs),
                                       ip(st.q_ptr), ip(st.q_pairs), B, Bv, Bw, Ti, Nq, D, fpm(dfv), fpm(dfw_total), fpm(dfs_total), wsp.data_ptr(),
                                       (size_t)wsp.numel()));
        keep.push_back(dfs_p); keep.push_back(dfw_p);
        venc_fs = at::ones({(int64_t)Bv, (int64_t)D}, opt);
        keep.push_back(venc_fs);
        df = dfv;
    }

    // the video encoder's input half, and where the three chains of the tail meet: the sums of the d f_s and d f_w parts
    void video_encoder_inputs()
    {
        SMIN_CK(smin_video_encoder_bwd(cur(), fp(df), fp(st.fv), fp(venc_fs), fp(st.vmaskf), fp(st.vx), Bv, Ti, Din, D, nullptr, nullptr, nullptr, fpm(dfs_video),
                                       wsv.data_ptr(), (size_t)wsv.numel()));
        if (!pairs) {
            dfs_parts.push_back(dfs_video);
            if (wordst != curs) await(curs, words_done);
            dfs_total = sum_list(dfs_parts); dfw_total = sum_list(dfw_parts);
        }
    }

    // f_s = [f_w[b, len_b - 1, :H] | f_w[b, 0, H:]] (models.py:60-62); then the video encoder's weight half on `bstr`
    void sentence_feature()
    {
        SMIN_CK(smin_sentence_feature_bwd(cur(), fp(dfs_total), ip(st.len32), Bw, Nq, i32(H), fpm(dfw_total)));
        dH = Nq_in < Nq ? dfw_total.slice(1, 0, Nq_in).contiguous() : dfw_total;
        keep.push_back(dfs_total); keep.push_back(dfw_total); keep.push_back(dH); keep.push_back(df); keep.push_back(dfs_video);
        wait_stream(bstr, curs);
        StreamScope sc(bstr);
        SMIN_CK(smin_video_encoder_bwd(cur(), nullptr, fp(st.fv), fp(venc_fs), fp(st.vmaskf), fp(st.vx), Bv, Ti, Din, D, fpm(dprm.backbone(P_VE_W)), fpm(dprm.backbone(P_VE_B)),
                                       fpm(dprm.backbone(P_PE)), nullptr, wsv.data_ptr(), (size_t)wsv.numel()));
    }

    void lstm_layer(int layer)
    {
        LstmState& ls = st.lstm[layer];
        const int In = i32(ls.x.size(2)), Hh = i32(H);
        Tensor dX = layer > 0 || want_dX ? at::empty_like(ls.x) : Tensor();
        Tensor dWih = at::empty_like(ls.Wih), dbias = at::empty({8 * H}, opt), dWhh = at::empty_like(ls.Whh);
        lstm_bufs.push_back(dWih); lstm_bufs.push_back(dbias); lstm_bufs.push_back(dWhh);
        Tensor wsl = own(smin_bilstm_layer_bwd_workspace_bytes(Bw, i32(Nq_in), In, Hh));
        SMIN_CK(smin_bilstm_layer_bwd(cur(), fp(dH), fp(ls.x), fp(ls.Hout), fp(ls.G), fp(ls.Cs), fp(tr[tr_tail + 1 + layer]), fp(ls.Whh), ip(st.len32), Bw, i32(Nq_in), In, Hh,
                                      fpm(dX), nullptr, nullptr, nullptr, wsl.data_ptr(), (size_t)wsl.numel()));
        // the weight gradients: three independent pieces; the last layer's (nothing else is left to run by then) on three streams,
        // pieces that share a stream in one call.  b_ih and b_hh get the same gradient in two tensors (dbias2: one tensor handed
        // to both made autograd clone it, a launch per bias at the very end of the step).
        Tensor dbias2 = at::empty({8 * H}, opt);
        lstm_bufs.push_back(dbias2);
        HStream piece[3] = {bstr, bstr, bstr};
        if (layer == 0 && bstr == wordst && tail != curs) { piece[1] = tail; piece[2] = wstr; }
        for (int pc = 0; pc < 3; ++pc) {
            int which = 1 << pc;
            while (pc + 1 < 3 && piece[pc + 1] == piece[pc]) which |= 1 << ++pc;
            wait_stream(piece[pc], curs);
            StreamScope sc(piece[pc]);
            SMIN_CK(smin_bilstm_layer_bwd_weights(cur(), which, fp(ls.x), fp(ls.Hout), Bw, i32(Nq_in), In, Hh, fpm(dWih), fpm(dbias), fpm(dbias2), fpm(dWhh),
                                                  wsl.data_ptr(), (size_t)wsl.numel()));
        }
        if (dX.defined()) keep.push_back(dX);
        const int64_t H4 = 4 * H;
        Tensor* o = &dprm.backbone(P_LSTM + 8 * layer);
        o[0] = dWih.slice(0, 0, H4); o[1] = dWhh[0]; o[2] = dbias.slice(0, 0, H4); o[3] = dbias2.slice(0, 0, H4);
        o[4] = dWih.slice(0, H4); o[5] = dWhh[1]; o[6] = dbias.slice(0, H4); o[7] = dbias2.slice(0, H4);
        dH = dX;
    }

    // the video features' gradient behind the last recurrence, on the main stream: the cluster recurrences need every CU's LDS
    // co-resident, and here only the layer-0 weight pieces are left beside it (measured against the weight stream: DESIGN 6)
    void input_gradients()
    {
        dquery = dH;
        if (want_dx) {
            dvideo = at::empty_like(st.vx);
            SMIN_CK(smin_video_encoder_bwd_input(cur(), fp(tr[tr_tail + 3]), fp(st.vmaskf), Bv, Ti, Din, D, fpm(dvideo), wsv.data_ptr(), (size_t)wsv.numel()));
        }
    }

    // every stream back into the caller's; then the backbone's gradients to the exchange
    void join()
    {
        wait_stream(curs, tail);
        wait_stream(curs, wstr);
        wait_stream(curs, wordst);
        if (sync.on) {
            std::vector<Tensor> late{dprm.backbone(P_VE_W), dprm.backbone(P_VE_B), dprm.backbone(P_PE)};
            for (auto& t : lstm_bufs) late.push_back(t);
            sync.reduce(late, curs);
            sync.join(curs);
        }
    }

    variable_list result()
    {
        variable_list out(N_FIXED + dprm.all.size());
        if (want_dx) out[0] = dvideo;
        if (want_dX) out[1] = dquery;
        std::copy(dprm.all.begin(), dprm.all.end(), out.begin() + N_FIXED);
        return out;
    }
};

}  // namespace
