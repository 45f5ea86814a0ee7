// The loss nodes of the torch extension: the restated training loss and the two losses over a pair plan.
#pragma once
#include "binding_util.h"

namespace {

// restated loss of the reference's train loop (main.py:89-116): one forward and one backward kernel
struct LossNode : torch::autograd::Function<LossNode> {
    static Tensor forward(AutogradContext* ctx, Tensor pm, Tensor ps, Tensor pe, Tensor pa, Tensor ym, Tensor sm, Tensor mm, Tensor ys, Tensor ss, Tensor ye, Tensor se,
                          Tensor ya, Tensor lm)
    {
        auto f = [](const Tensor& t) { return cont(fl(t)); };
        auto b = [](const Tensor& t) { return cont((t.scalar_type() == at::kBool || t.scalar_type() == at::kByte) ? t : t.ne(0)); };
        pm = f(pm); ps = f(ps); pe = f(pe); pa = f(pa); sm = f(sm); ss = f(ss); se = f(se);
        ym = b(ym); mm = b(mm); ys = b(ys); ye = b(ye); ya = b(ya); lm = b(lm);
        const int B = i32(ps.size(0)), L = i32(ps.size(1));
        Tensor loss = at::empty({1}, pm.options()), part = at::empty({B, 6}, pm.options());
        SMIN_CK(smin_loss_fwd(cur(), fp(pm), u8(ym), fp(sm), u8(mm), fp(ps), u8(ys), fp(ss), fp(pe), u8(ye), fp(se), fp(pa), u8(ya), u8(lm), B, L, fpm(loss), fpm(part)));
        ctx->save_for_backward({pm, ps, pe, pa, ym, sm, mm, ys, ss, ye, se, ya, lm, part});
        return loss.reshape({});
    }
    static variable_list backward(AutogradContext* ctx, variable_list g)
    {
        auto sv = ctx->get_saved_variables();
        const Tensor &pm = sv[0], &ps = sv[1], &pe = sv[2], &pa = sv[3], &ym = sv[4], &sm = sv[5], &mm = sv[6], &ys = sv[7], &ss = sv[8], &ye = sv[9], &se = sv[10],
                     &ya = sv[11], &lm = sv[12], &part = sv[13];
        const int B = i32(ps.size(0)), L = i32(ps.size(1));
        Tensor dloss = cont(fl(g[0].reshape({1})));
        // the three score gradients are rows of one buffer: the model's node takes them as they are (no gather)
        Tensor dpm = at::empty_like(pm), d3 = at::empty({3, (int64_t)B, (int64_t)L}, ps.options());
        Tensor dps = d3[0], dpe = d3[1], dpa = d3[2];
        SMIN_CK(smin_loss_bwd(cur(), fp(dloss), fp(part), fp(pm), u8(ym), fp(sm), u8(mm), fp(ps), u8(ys), fp(ss), fp(pe), u8(ye), fp(se), fp(pa), u8(ya), u8(lm), B, L,
                              fpm(dpm), fpm(dps), fpm(dpe), fpm(dpa)));
        variable_list out{dpm, dps, dpe, dpa};
        for (int k = 0; k < 9; ++k) out.push_back(undef());
        return out;
    }
};


// What the two losses over a pair plan share (csrc/pair_rank.hip): the operands as the kernels read them, the forward's outputs, what
// it saves, and the one backward launch.  `extra` is the node's own operand: the positives (int32), or with soft = true a teacher's scores.
struct PairLossCall {
    Tensor pm, ps, pe, mm, q_ptr, q_pairs, extra, loss, stats, score, coef, pool;
    int P, L, Q;
    PairLossCall(const Tensor& pm_, const Tensor& ps_, const Tensor& pe_, const Tensor& mm_, const Tensor& q_ptr_, const Tensor& q_pairs_, const Tensor& extra_, bool soft)
    {
        auto i = [](const Tensor& t) { return cont(t.scalar_type() == at::kInt ? t : t.to(at::kInt)); };
        pm = cont(fl(pm_)); ps = cont(fl(ps_)); pe = cont(fl(pe_));
        if (soft) extra = cont(fl(extra_.detach()));
        mm = cont((mm_.scalar_type() == at::kBool || mm_.scalar_type() == at::kByte) ? mm_ : mm_.ne(0));
        q_ptr = i(q_ptr_); q_pairs = i(q_pairs_);
        if (!soft) extra = i(extra_);
        P = i32(ps.size(0)); L = i32(ps.size(1)); Q = i32(q_ptr.size(0) - 1);
        loss = at::empty({1}, pm.options()); stats = at::empty({2}, pm.options()); score = at::empty({(int64_t)P}, pm.options());
        coef = at::empty({(int64_t)P}, pm.options()); pool = at::empty({(int64_t)P, 2}, pm.options());
    }
    variable_list finish(AutogradContext* ctx, double tau)
    {
        ctx->save_for_backward({pm, ps, pe, mm, stats, coef, pool});
        ctx->saved_data["tau"] = tau;
        ctx->mark_non_differentiable({stats, score});
        return {loss.reshape({}), stats, score};
    }
    // gradients to pm, ps, pe; `inputs`: the number of the node's forward arguments
    static variable_list backward(AutogradContext* ctx, const variable_list& g, int inputs)
    {
        auto sv = ctx->get_saved_variables();
        const Tensor &pm = sv[0], &ps = sv[1], &pe = sv[2], &mm = sv[3], &stats = sv[4], &coef = sv[5], &pool = sv[6];
        const int P = i32(ps.size(0)), L = i32(ps.size(1));
        Tensor dloss = cont(fl(g[0].reshape({1})));
        Tensor dpm = at::empty_like(pm), dps = at::empty_like(ps), dpe = at::empty_like(pe);
        SMIN_CK(smin_pair_rank_bwd(cur(), fp(dloss), fp(stats), fp(coef), fp(pool), fp(pm), fp(ps), fp(pe), u8(mm), P, L, (float)ctx->saved_data["tau"].toDouble(),
                                   fpm(dpm), fpm(dps), fpm(dpe)));
        variable_list out{dpm, dps, dpe};
        for (int k = 3; k < inputs; ++k) out.push_back(undef());
        return out;
    }
};

// video-level contrastive loss over a pair plan: three forward launches, one backward launch
struct PairRankNode : torch::autograd::Function<PairRankNode> {
    static variable_list forward(AutogradContext* ctx, Tensor pm, Tensor ps, Tensor pe, Tensor mm, Tensor q_ptr, Tensor q_pairs, Tensor positive, double tau,
                                 double gamma)
    {
        PairLossCall c(pm, ps, pe, mm, q_ptr, q_pairs, positive, false);
        Scratch ws = scratch(smin_pair_rank_ws_bytes(c.P, c.Q, c.L), c.pm.device());
        SMIN_CK(smin_pair_rank_fwd(cur(), fp(c.pm), fp(c.ps), fp(c.pe), u8(c.mm), ip(c.q_ptr), ip(c.q_pairs), ip(c.extra), c.P, c.Q, c.L, (float)tau, (float)gamma,
                                   fpm(c.loss), fpm(c.stats), fpm(c.score), fpm(c.coef), fpm(c.pool), ws.p, ws.n));
        return c.finish(ctx, tau);
    }
    static variable_list backward(AutogradContext* ctx, variable_list g) { return PairLossCall::backward(ctx, g, 9); }
};

// listwise soft-target loss over a pair plan: three forward launches, PairRankNode's backward call
struct PairDistillNode : torch::autograd::Function<PairDistillNode> {
    static variable_list forward(AutogradContext* ctx, Tensor pm, Tensor ps, Tensor pe, Tensor mm, Tensor q_ptr, Tensor q_pairs, Tensor teacher, double tau,
                                 double gamma, double gamma_teacher)
    {
        PairLossCall c(pm, ps, pe, mm, q_ptr, q_pairs, teacher, true);
        Scratch ws = scratch(smin_pair_distill_ws_bytes(c.P, c.Q, c.L), c.pm.device());
        SMIN_CK(smin_pair_distill_fwd(cur(), fp(c.pm), fp(c.ps), fp(c.pe), u8(c.mm), ip(c.q_ptr), ip(c.q_pairs), fp(c.extra), c.P, c.Q, c.L, (float)tau, (float)gamma,
                                      (float)gamma_teacher, fpm(c.loss), fpm(c.stats), fpm(c.score), fpm(c.coef), fpm(c.pool), ws.p, ws.n));
        return c.finish(ctx, tau);
    }
    static variable_list backward(AutogradContext* ctx, variable_list g) { return PairLossCall::backward(ctx, g, 10); }
};

}  // namespace
