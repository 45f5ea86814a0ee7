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
#include <ATen/ATen.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <ATen/core/stack.h>

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "smin_hip.h"

namespace {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;
using HStream = c10::hip::HIPStream;

#define SMIN_CK(call)                                                                           \
    do {                                                                                        \
        const int rc__ = (call);                                                                \
        TORCH_CHECK(rc__ == 0, "smin_hip: " #call " failed with code ", rc__,                   \
                    rc__ < -1000 ? " (argument rejected at csrc line " + std::to_string(-rc__ - 1000) + ")" : std::string()); \
    } while (0)

// ---------------------------------------------------------------- small helpers
inline const float* fp(const Tensor& t) { return t.defined() ? t.const_data_ptr<float>() : nullptr; }
inline float* fpm(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
inline const uint16_t* hp16(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.const_data_ptr()); }     // bf16 tensors as bit patterns
inline const int32_t* ip(const Tensor& t) { return t.const_data_ptr<int32_t>(); }
inline const uint8_t* u8(const Tensor& t) { return static_cast<const uint8_t*>(t.const_data_ptr()); }             // one-byte masks
inline void* cur() { return (void*)c10::hip::getCurrentHIPStream().stream(); }
inline Tensor cont(const Tensor& t) { return t.defined() ? t.contiguous() : t; }
inline Tensor fl(const Tensor& t) { return t.scalar_type() == at::kFloat ? t : t.to(at::kFloat); }
inline int i32(int64_t v) { return static_cast<int>(v); }

struct StreamScope {                       // torch's current stream for the scope (what torch.cuda.stream(s) does)
    HStream prev;
    explicit StreamScope(HStream s) : prev(c10::hip::getCurrentHIPStream(s.device_index())) { c10::hip::setCurrentHIPStream(s); }
    ~StreamScope() { c10::hip::setCurrentHIPStream(prev); }
};

// The process-wide caches below: a map under its own lock (the forward runs on the caller's thread, the backward on the autograd
// engine's).  get() returns the key's entry, made by `make` under the lock the first time; entries are never erased.
template <class K, class V>
struct Cache {
    std::mutex mu;
    std::map<K, V> m;
    template <class Make> V& get(const K& key, Make make)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = m.find(key);
        if (it == m.end()) it = m.emplace(key, make()).first;
        return it->second;
    }
};

// Events for stream joins: a ring per device (an event is bound to the device it was created on), created under that device's
// guard.  A draw is consumed (marked and awaited by a stream, or waited for by the host) within the call that
// drew it; the ring is far longer than the draws of one forward + backward pass (~60 at three layers), so no event is
// re-recorded while a wait on its previous record is still being enqueued.
hipEvent_t next_event()
{
    constexpr size_t RING = 1024;
    static Cache<int, std::pair<std::vector<hipEvent_t>, size_t>> rings;   // (its draw counter advances: locked here)
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice failed");
    std::lock_guard<std::mutex> lk(rings.mu);
    auto& ring = rings.m[dev];
    if (ring.first.empty()) {
        ring.first.resize(RING);
        for (auto& e : ring.first) TORCH_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
    }
    return ring.first[ring.second++ % RING];
}
// The two verbs of every hand-off between streams (the rules that make them safe: DESIGN.md 6, "Stream rules"):
// mark: an event behind everything queued on `on` so far; await: `waiter` runs nothing further until `e` has happened
hipEvent_t mark(HStream on)
{
    hipEvent_t e = next_event();
    TORCH_CHECK(hipEventRecord(e, on.stream()) == hipSuccess, "hipEventRecord failed");
    return e;
}
void await(HStream waiter, hipEvent_t e) { TORCH_CHECK(hipStreamWaitEvent(waiter.stream(), e, 0) == hipSuccess, "hipStreamWaitEvent failed"); }
void host_wait(hipEvent_t e) { TORCH_CHECK(hipEventSynchronize(e) == hipSuccess, "hipEventSynchronize failed"); }
// `waiter` waits for everything queued on `on` so far (stream.wait_stream)
void wait_stream(HStream waiter, HStream on)
{
    if (waiter != on) await(waiter, mark(on));
}
HStream side_stream(c10::DeviceIndex dev, int which = 0)
{
    static Cache<std::pair<int, int>, HStream> streams;
    return streams.get({(int)dev, which}, [&] {
        HStream st = c10::hip::getStreamFromPool(false, dev);
        for (auto& kv : streams.m)                                // the pool hands its streams out round robin: never the same one twice
            while (kv.first.first == (int)dev && kv.second == st) st = c10::hip::getStreamFromPool(false, dev);
        return st;
    });
}

// lowest-priority stream for work nobody waits for until the end of the step (weight-gradient contractions)
HStream weight_stream(c10::DeviceIndex dev)
{
    static Cache<int, HStream> streams;
    return streams.get(dev, [&] {
        int least = 0, greatest = 0;
        TORCH_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess, "hipDeviceGetStreamPriorityRange failed");
        hipStream_t raw;
        TORCH_CHECK(hipStreamCreateWithPriority(&raw, hipStreamNonBlocking, least) == hipSuccess, "hipStreamCreateWithPriority failed");
        return c10::hip::getStreamFromExternal(raw, dev);
    });
}

// persistent scratch per (device, stream): calls on one stream are stream-ordered, two streams never share scratch.
// .n is the size that was asked for, not the buffer's capacity: an entry point's own check then sees an under-sized request on
// every call, not only on a fresh stream.
struct Scratch { void* p; size_t n; Tensor hold; };
Scratch scratch(size_t nbytes, const at::Device& dev)
{
    static Cache<std::pair<int, int64_t>, Tensor> bufs;                 // (an entry grows: locked here)
    const auto st = c10::hip::getCurrentHIPStream(dev.index());
    // A captured graph keeps the pointer it is given, and the persistent buffer is replaced (and freed) by the next larger request:
    // inside a capture the scratch comes from the graph's own memory pool, like every other tensor of the captured step.
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    TORCH_CHECK(hipStreamIsCapturing(st.stream(), &capture) == hipSuccess, "hipStreamIsCapturing failed");
    if (capture != hipStreamCaptureStatusNone) {
        Tensor t = at::empty({(int64_t)std::max<size_t>(nbytes, 16)}, at::TensorOptions().dtype(at::kByte).device(dev));
        return Scratch{t.data_ptr(), nbytes, t};
    }
    std::lock_guard<std::mutex> lk(bufs.mu);
    Tensor& b = bufs.m[{(int)dev.index(), (int64_t)st.id()}];
    if (!b.defined() || (size_t)b.numel() < nbytes)
        b = at::empty({(int64_t)(nbytes + nbytes / 4 + 4096)}, at::TensorOptions().dtype(at::kByte).device(dev));
    return Scratch{b.data_ptr(), nbytes, b};
}
// scratch of the size an entry point's own query returns (0 = the entry point would reject these shape arguments):
// SMIN_WS(smin_gate_bwd_ws_bytes(B, L, D), dev)
Scratch scratch_for(size_t need, const char* query, const at::Device& dev)
{
    TORCH_CHECK(need > 0, query, " rejected its arguments");
    return scratch(need, dev);
}
#define SMIN_WS(query_call, dev) scratch_for(query_call, #query_call, dev)

// the geometry's clip-boundary table, built once per (device, T, L, C)
std::pair<Tensor, Tensor> clip_event_table(const at::Device& dev, int T, int L, int C, bool* built_now = nullptr)
{
    static Cache<std::tuple<int, int, int, int>, std::pair<Tensor, Tensor>> tabs;
    bool built = false;
    auto& tab = tabs.get(std::make_tuple((int)dev.index(), T, L, C), [&] {
        built = true;
        auto io = at::TensorOptions().dtype(at::kInt).device(dev);
        Tensor counts = at::empty({T}, io);
        SMIN_CK(smin_clip_event_table(cur(), T, L, C, counts.data_ptr<int32_t>(), nullptr, nullptr));
        Tensor offsets = at::zeros({T + 1}, io);
        offsets.slice(0, 1).copy_(at::cumsum(counts, 0).to(at::kInt));
        const int64_t n = std::max<int64_t>(1, offsets[T].item<int64_t>());
        Tensor table = at::empty({n, 2}, io);
        SMIN_CK(smin_clip_event_table(cur(), T, L, C, nullptr, ip(offsets), table.data_ptr()));
        return std::make_pair(offsets, table);
    });
    if (built_now) *built_now = built;                            // built on the CURRENT stream: a consumer on another stream has to wait for it
    return tab;
}

Tensor undef() { return Tensor(); }

// device word that smin_build_cells_n sets when a caller-supplied cell count does not match the mask (see csrc/layout.hip)
Tensor layout_status(const at::Device& dev)
{
    static Cache<int, Tensor> st;
    return st.get(dev.index(), [&] { return at::zeros({1}, at::TensorOptions().dtype(at::kInt).device(dev)); });
}

// the two device words smin_step_prologue counts with (zero between launches)
Tensor prologue_words(const at::Device& dev)
{
    static Cache<int, Tensor> st;
    return st.get(dev.index(), [&] { return at::zeros({2}, at::TensorOptions().dtype(at::kLong).device(dev)); });
}

// ---------------------------------------------------------------- gradient exchange inside the node (data parallel)
// With the whole model as one autograd node torch DDP sees every gradient only when the node returns: its all-reduce would start
// after the backward pass.  Instead the node hands each group of finished gradient buffers to the process group itself
// (c10d functional collectives, i.e. RCCL on a HIP device), on the stream that produced them, as soon as they are final -- the
// boundary unit's and moment unit's weights layer by layer, the inputs of the parameter-product kernel before it runs (its outputs
// are linear in them with coefficients that are equal on every rank, so they come out averaged), the word-side and localization
// gradients behind their kernels, the backbone's at the end -- and the main stream joins the collectives before the node returns.
struct GradSyncConfig { std::string group; int world = 1; bool coalesced_avg = false; };
GradSyncConfig& grad_sync_config() { static GradSyncConfig c; return c; }

struct GradSync {
    bool on = false;
    std::vector<Tensor> pending;
    static c10::OperatorHandle op(const char* name) { return c10::Dispatcher::singleton().findSchemaOrThrow(name, ""); }
    // every tensor: a contiguous gradient buffer, handed over exactly once; `on_stream` = the stream its producer ran on
    void reduce(const std::vector<Tensor>& ts_in, HStream on_stream)
    {
        if (!on) return;
        std::vector<Tensor> ts;
        for (auto& t : ts_in) if (t.defined() && t.numel() > 0) { TORCH_CHECK(t.is_contiguous(), "grad sync: non-contiguous gradient buffer"); ts.push_back(t); }
        if (ts.empty()) return;
        const GradSyncConfig& c = grad_sync_config();
        StreamScope sc(on_stream);
        if (c.coalesced_avg) {                                   // RCCL: one grouped launch, averaged by the library
            static auto h = op("_c10d_functional::all_reduce_coalesced_");
            torch::jit::Stack stack;
            stack.emplace_back(ts); stack.emplace_back(std::string("avg")); stack.emplace_back(c.group);
            h.callBoxed(stack);
            for (auto& t : ts) pending.push_back(t);
        } else {                                                  // gloo (tests): per tensor, summed, then scaled
            static auto h = op("_c10d_functional::all_reduce_");
            static auto w = op("_c10d_functional::wait_tensor");
            for (auto& t : ts) {
                torch::jit::Stack stack;
                stack.emplace_back(t); stack.emplace_back(std::string("sum")); stack.emplace_back(c.group);
                h.callBoxed(stack);
                torch::jit::Stack ws; ws.emplace_back(t);
                w.callBoxed(ws);
                t.mul_(1.0 / c.world);
            }
        }
    }
    // `waiter` waits for every collective handed over so far
    void join(HStream waiter)
    {
        if (pending.empty()) return;
        static auto w = op("_c10d_functional::wait_tensor");
        StreamScope sc(waiter);
        for (auto& t : pending) { torch::jit::Stack ws; ws.emplace_back(t); w.callBoxed(ws); }
        pending.clear();
    }
};

// parameter order (modules.py: SMIN._native_params): video encoder 3, LSTM 16, 20 per SMI layer, localization 8
enum { P_VE_W = 0, P_VE_B, P_PE, P_LSTM = 3, P_LAYER0 = 19 };
enum { L_CH_W = 0, L_CH_B, L_WH_W, L_WH_B, L_SH_W, L_SH_B, L_C_W, L_C_B, L_AQ_W, L_AQ_B, L_AK_W, L_AK_B, L_BQ_W, L_BQ_B, L_BK_W, L_BK_B, L_FB_W, L_FB_B, L_FC_W,
       L_FC_B, L_COUNT };
// a layer's parameters that meet in the parameter products (csrc/param_prep.hip), and its word-side ones (csrc/word_prep.hip)
constexpr int L_PRODUCTS[] = {L_CH_W, L_CH_B, L_C_W, L_C_B, L_FB_W, L_FB_B, L_FC_W, L_FC_B}, L_WORD_SIDE[] = {L_WH_W, L_WH_B, L_SH_W, L_SH_B, L_AK_W, L_AK_B, L_AQ_W, L_AQ_B};
// The contiguous parameters of a run, or their gradients (ParamList(nl): undefined until formed), under one index arithmetic.
struct ParamList {
    std::vector<Tensor> all;
    int64_t nl = 0;
    static int64_t expected(int64_t nl) { return P_LAYER0 + nl * L_COUNT + 8; }
    ParamList() = default;
    explicit ParamList(int64_t nl) : all(expected(nl)), nl(nl) {}
    ParamList(std::vector<Tensor> ts, int64_t nl) : all(std::move(ts)), nl(nl) {}
    ParamList(at::TensorList ts, size_t count, int64_t nl) : nl(nl) { for (size_t i = 0; i < count; ++i) all.push_back(cont(ts[i])); }
    const Tensor& backbone(int which) const { return all[which]; }                       // P_VE_W .. P_LSTM + 15
    Tensor& backbone(int which) { return all[which]; }
    const Tensor& layer(int64_t k, int which) const { return all[P_LAYER0 + k * L_COUNT + which]; }
    Tensor& layer(int64_t k, int which) { return all[P_LAYER0 + k * L_COUNT + which]; }
    const Tensor& loc(int i) const { return all[P_LAYER0 + nl * L_COUNT + i]; }           // the localization head's 8
    Tensor& loc(int i) { return all[P_LAYER0 + nl * L_COUNT + i]; }
};

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


// video-level contrastive loss over a pair plan (csrc/pair_rank.hip): three forward launches, one backward launch
struct PairRankNode : torch::autograd::Function<PairRankNode> {
    static variable_list forward(AutogradContext* ctx, Tensor pm, Tensor ps, Tensor pe, Tensor mm, Tensor q_ptr, Tensor q_pairs, Tensor positive, double tau,
                                 double gamma)
    {
        auto i = [](const Tensor& t) { return cont(t.scalar_type() == at::kInt ? t : t.to(at::kInt)); };
        pm = cont(fl(pm)); ps = cont(fl(ps)); pe = cont(fl(pe));
        mm = cont((mm.scalar_type() == at::kBool || mm.scalar_type() == at::kByte) ? mm : mm.ne(0));
        q_ptr = i(q_ptr); q_pairs = i(q_pairs); positive = i(positive);
        const int P = i32(ps.size(0)), L = i32(ps.size(1)), Q = i32(q_ptr.size(0) - 1);
        Tensor loss = at::empty({1}, pm.options()), stats = at::empty({2}, pm.options()), score = at::empty({(int64_t)P}, pm.options());
        Tensor coef = at::empty({(int64_t)P}, pm.options()), pool = at::empty({(int64_t)P, 2}, pm.options());
        const size_t need = smin_pair_rank_ws_bytes(P, Q, L);
        Scratch ws = scratch(need, pm.device());
        SMIN_CK(smin_pair_rank_fwd(cur(), fp(pm), fp(ps), fp(pe), u8(mm), ip(q_ptr), ip(q_pairs), ip(positive), P, Q, L, (float)tau, (float)gamma, fpm(loss),
                                   fpm(stats), fpm(score), fpm(coef), fpm(pool), ws.p, ws.n));
        ctx->save_for_backward({pm, ps, pe, mm, stats, coef, pool});
        ctx->saved_data["tau"] = tau;
        ctx->mark_non_differentiable({stats, score});
        return {loss.reshape({}), stats, score};
    }
    static variable_list backward(AutogradContext* ctx, variable_list g)
    {
        auto sv = ctx->get_saved_variables();
        const Tensor &pm = sv[0], &ps = sv[1], &pe = sv[2], &mm = sv[3], &stats = sv[4], &coef = sv[5], &pool = sv[6];
        const int P = i32(ps.size(0)), L = i32(ps.size(1));
        Tensor dloss = cont(fl(g[0].reshape({1})));
        Tensor dpm = at::empty_like(pm), dps = at::empty_like(ps), dpe = at::empty_like(pe);
        SMIN_CK(smin_pair_rank_bwd(cur(), fp(dloss), fp(stats), fp(coef), fp(pool), fp(pm), fp(ps), fp(pe), u8(mm), P, L, (float)ctx->saved_data["tau"].toDouble(),
                                   fpm(dpm), fpm(dps), fpm(dpe)));
        variable_list out{dpm, dps, dpe};
        for (int k = 0; k < 6; ++k) out.push_back(undef());
        return out;
    }
};


// listwise soft-target loss over a pair plan (csrc/pair_rank.hip): three forward launches, PairRankNode's backward call
struct PairDistillNode : torch::autograd::Function<PairDistillNode> {
    static variable_list forward(AutogradContext* ctx, Tensor pm, Tensor ps, Tensor pe, Tensor mm, Tensor q_ptr, Tensor q_pairs, Tensor teacher, double tau,
                                 double gamma, double gamma_teacher)
    {
        auto i = [](const Tensor& t) { return cont(t.scalar_type() == at::kInt ? t : t.to(at::kInt)); };
        pm = cont(fl(pm)); ps = cont(fl(ps)); pe = cont(fl(pe)); teacher = cont(fl(teacher.detach()));
        mm = cont((mm.scalar_type() == at::kBool || mm.scalar_type() == at::kByte) ? mm : mm.ne(0));
        q_ptr = i(q_ptr); q_pairs = i(q_pairs);
        const int P = i32(ps.size(0)), L = i32(ps.size(1)), Q = i32(q_ptr.size(0) - 1);
        Tensor loss = at::empty({1}, pm.options()), stats = at::empty({2}, pm.options()), score = at::empty({(int64_t)P}, pm.options());
        Tensor coef = at::empty({(int64_t)P}, pm.options()), pool = at::empty({(int64_t)P, 2}, pm.options());
        const size_t need = smin_pair_distill_ws_bytes(P, Q, L);
        Scratch ws = scratch(need, pm.device());
        SMIN_CK(smin_pair_distill_fwd(cur(), fp(pm), fp(ps), fp(pe), u8(mm), ip(q_ptr), ip(q_pairs), fp(teacher), P, Q, L, (float)tau, (float)gamma,
                                      (float)gamma_teacher, fpm(loss), fpm(stats), fpm(score), fpm(coef), fpm(pool), ws.p, ws.n));
        ctx->save_for_backward({pm, ps, pe, mm, stats, coef, pool});
        ctx->saved_data["tau"] = tau;
        ctx->mark_non_differentiable({stats, score});
        return {loss.reshape({}), stats, score};
    }
    static variable_list backward(AutogradContext* ctx, variable_list g)
    {
        auto sv = ctx->get_saved_variables();
        const Tensor &pm = sv[0], &ps = sv[1], &pe = sv[2], &mm = sv[3], &stats = sv[4], &coef = sv[5], &pool = sv[6];
        const int P = i32(ps.size(0)), L = i32(ps.size(1));
        Tensor dloss = cont(fl(g[0].reshape({1})));
        Tensor dpm = at::empty_like(pm), dps = at::empty_like(ps), dpe = at::empty_like(pe);
        SMIN_CK(smin_pair_rank_bwd(cur(), fp(dloss), fp(stats), fp(coef), fp(pool), fp(pm), fp(ps), fp(pe), u8(mm), P, L, (float)ctx->saved_data["tau"].toDouble(),
                                   fpm(dpm), fpm(dps), fpm(dpe)));
        variable_list out{dpm, dps, dpe};
        for (int k = 0; k < 7; ++k) out.push_back(undef());
        return out;
    }
};


// ---------------------------------------------------------------- the fused core
// ProposalGeneration + every SMI layer + Localization (models.py:101-126, 306-344) as ONE autograd node: forward and backward
// are straight-line sequences of the C entry points with hand-placed stream forks.  What a node per module (the Python host's
// graph) pays and this does not: ~60 engine node visits, the engine's out-of-place sums for every tensor with several consumers
// (f_s, f_w, the boundary features, the parameters shared between layers -- ~45 tiny launches per step), a transposed copy per
// weight per backward call (one batched launch here) and the autograd bookkeeping of the parameter products.
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

// W^T of every listed matrix, one launch per 32 matrices
std::vector<Tensor> transpose_all(const std::vector<Tensor>& ws)
{
    std::vector<Tensor> out;
    for (size_t lo = 0; lo < ws.size(); lo += SMIN_BATCH_MAX) {
        const size_t n = std::min(ws.size() - lo, (size_t)SMIN_BATCH_MAX);
        const float* src[SMIN_BATCH_MAX]; float* dst[SMIN_BATCH_MAX]; int32_t rows[SMIN_BATCH_MAX], cols[SMIN_BATCH_MAX];
        for (size_t m = 0; m < n; ++m) {
            const Tensor& w = ws[lo + m];
            TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "transpose_all: contiguous matrices only");
            out.push_back(at::empty({w.size(1), w.size(0)}, w.options()));
            src[m] = fp(w); dst[m] = fpm(out.back()); rows[m] = i32(w.size(0)); cols[m] = i32(w.size(1));
        }
        SMIN_CK(smin_transpose_batch(cur(), src, dst, rows, cols, i32(n)));
    }
    return out;
}
Tensor sum_list(const std::vector<Tensor>& ts)
{
    TORCH_CHECK(!ts.empty() && ts.size() <= SMIN_BATCH_MAX, "sum_list: 1..", SMIN_BATCH_MAX, " tensors");
    if (ts.size() == 1) return ts[0];
    const float* p[SMIN_BATCH_MAX];
    for (size_t k = 0; k < ts.size(); ++k) { TORCH_CHECK(ts[k].is_contiguous() && ts[k].numel() == ts[0].numel(), "sum_list: shapes differ"); p[k] = fp(ts[k]); }
    Tensor out = at::empty_like(ts[0]);
    SMIN_CK(smin_sum_lists(cur(), p, i32(ts.size()), (size_t)ts[0].numel(), fpm(out)));
    return out;
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

struct SminCore : torch::autograd::Function<SminCore> {
    enum { N_FIXED = 3 };           // forward arguments ahead of the parameter list: video_features, query_features, the call (one gradient slot each)

    // The forward pass as a sequence of launches, for the node's forward (scoring = false: every tensor the backward reads stays in `st`)
    // and for smin_score (scoring = true: forward only -- a layer's tensors are dropped once their last reader is queued, and the last
    // layer ends in smin_score_tail_fwd instead of its content-stream sum, pair product, moment unit and smin_score_map_fwd).
    // Fills st.pm / st.psea, the contiguous parameters st.prm and the attention maps; returns the number of cells.
    // call.bank: the backbone's outputs of the pairs come from banks through smin_pair_assemble and the four masks are the pairs'.
    // Scoring: the banks are given and video_features / query_features are unused.  Training (bank->train): the two
    // encoders run here, once per row of video_features (V, T, Din) and of query_features (Q, words, E), and their state is kept.
    static int64_t run(CoreState& st, const CoreCall& call, const Tensor& video_features, const Tensor& query_features, at::TensorList prm_in)
    {
        const auto& [video_mask, query_mask, length_mask, moment_mask, T, L, C, nl, maxq, H, flags, n_known, scoring, given_bank] = call;
        const PairBank* bank = given_bank ? &*given_bank : nullptr;
        TORCH_CHECK(!bank || scoring != bank->train, "given banks are scored; a training run encodes its own");
        const bool own_bank = bank && bank->train;
        const ParamList& P = st.prm = ParamList(prm_in, prm_in.size(), nl);
        const Tensor& like = bank && !own_bank ? (bank->storage ? bank->fw : bank->fv) : video_features;     // (fp32: its options make the run's tensors)
        const int64_t Bq = bank ? bank->vi.size(0) : video_features.size(0), Tn = bank && !own_bank ? bank->fv.size(1) : like.size(1);
        TORCH_CHECK(Tn == T, "ProposalGeneration was built for T=", T, " but got ", Tn, " frames");
        const auto [dev, opt, B, D, Nq, dl, Li, Ci, Ti, curs, side] = Dims(like, Bq, P, T, L, C, maxq, flags);
        HStream prep = (flags & F_OVERLAP_PREP) ? side : curs;
        size_state(st, nl);

        // ---- parameter-only work (weight products, constants, concatenations: ~25 tiny launches) on the second stream from the first
        // moment of the step, beside the LSTM recurrence that opens the critical path; the main stream waits for it before the proposal map
        std::vector<Tensor> bcat(nl);
        Tensor bb;
        hipEvent_t products_ready;
        const bool prep_kernel = (flags & F_PARAM_PREP_KERNEL) != 0;                // csrc/param_prep.hip (else: torch calls)
        wait_stream(prep, curs);                                                    // (the optimizer's update of the parameters)
        {
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
        Tensor qm = query_mask.reshape({Bq, -1});
        auto bytes = [](const Tensor& t) { return t.element_size() == 1 && t.is_contiguous(); };
        const bool fast_prologue = bytes(video_mask) && bytes(qm) && bytes(length_mask) && bytes(moment_mask) && qm.size(1) == maxq && video_mask.numel() == Bq * Tn &&
                                   length_mask.numel() == Bq * L && moment_mask.numel() == Bq * L * L;
        Tensor mm, host_n, qmf, lmf;
        if (fast_prologue) {
            st.wb = at::empty({3, (int64_t)D}, opt); bb = at::empty({3}, opt);
            st.len32 = at::empty({Bq}, opt.dtype(at::kInt));
            qmf = at::empty({Bq, maxq}, opt); lmf = at::empty({Bq, L}, opt); st.vmaskf = at::empty({Bq * Tn}, opt);
            Tensor count = at::empty({1}, opt.dtype(at::kLong));
            const float* w3[3] = {fp(P.loc(2)), fp(P.loc(4)), fp(P.loc(6))};
            const float* b3[3] = {fp(P.loc(3)), fp(P.loc(5)), fp(P.loc(7))};
            SMIN_CK(smin_step_prologue(cur(), u8(qm), u8(video_mask), u8(length_mask), u8(moment_mask), w3, b3, B, Nq, Ti, Li, D, st.len32.data_ptr<int32_t>(), fpm(qmf),
                                       fpm(st.vmaskf), fpm(lmf), fpm(st.wb), fpm(bb), count.data_ptr<int64_t>(), prologue_words(dev).data_ptr()));
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
            st.vmaskf = cont(fl(video_mask.reshape({Bq * Tn})));
            qmf = cont(fl(qm)); lmf = cont(fl(length_mask));
        }
        hipEvent_t count_ready = mark(curs);

        // ---- the video encoder's projection (models.py:25-36) on the second stream, beside the query encoder: only its product with the
        // sentence feature (models.py:81-83) waits for the LSTM layers (the fused call sat behind them: ~90 us of the step's opening chain).
        // Queued behind the parameter products: ahead of them it runs beside the LSTM operand packing and the first recurrence and
        // stretches both (pack 20 -> 84 us, recurrence 87 -> 130 us: the opening chain 45 us longer, tools/gantt.sh).
        if (!bank || own_bank) {
            st.vx = cont(video_features);
            st.fv = at::empty({st.vx.size(0), T, (int64_t)D}, opt);
        }
        Tensor f = at::empty({Bq, T, (int64_t)D}, opt), fw, fs;
        hipEvent_t projection_ready = nullptr;
        if (!bank && prep != curs) {
            await(prep, count_ready);                                              // (vmaskf)
            StreamScope sc(prep);
            SMIN_CK(smin_video_encoder_fwd(cur(), fp(st.vx), fp(P.backbone(P_VE_W)), fp(P.backbone(P_VE_B)), fp(P.backbone(P_PE)), fp(st.vmaskf), nullptr, B, Ti,
                                           i32(st.vx.size(2)), D, fpm(st.fv), nullptr));
            projection_ready = mark(prep);
        }

        // ---- backbone (models.py:38-83): BiLSTM x 2, sentence feature, fused video encoder
        if (bank) {
            Tensor bfv = bank->fv, bfw = bank->fw, bfs = bank->fs;
            if (own_bank) {
                // the two encoders once per video and once per query, on the main stream (as smin_encode_videos / smin_encode_queries);
                // the prologue's vmaskf and len32 above are per pair and are replaced by the encoders' own rows, which the backward reads
                st.len32 = query_lengths(bank->qmask_q.reshape({query_features.size(0), -1}));
                st.vmaskf = project_videos(P, st.vx, bank->vmask_v.reshape({st.vx.size(0) * Tn}), st.fv);
                std::tie(bfw, bfs) = query_encoder(st.lstm, P, query_features, st.len32, maxq, H, false);
                bfv = st.fv;
                st.fs_bank = bfs; st.vi = bank->vi; st.qi = bank->qi;
                st.v_ptr = bank->v_ptr; st.v_pairs = bank->v_pairs; st.q_ptr = bank->q_ptr; st.q_pairs = bank->q_pairs;
            }
            // both encoders ran once per video and per query: the pairs' f = f_v * f_s, f_w and f_s in one launch (csrc/corpus.hip)
            fw = at::empty({Bq, maxq, (int64_t)D}, opt); fs = at::empty({Bq, (int64_t)D}, opt);
            if (bank->storage)
                SMIN_CK(smin_pair_assemble_compact(cur(), bfv.const_data_ptr(), bank->fv_scale.defined() ? fp(bank->fv_scale) : nullptr, bank->storage, fp(bfs), fp(bfw),
                                                   ip(bank->vi), ip(bank->qi), B, i32(bfv.size(0)), i32(bfs.size(0)), Ti, Nq, D, fpm(f), fpm(fw), fpm(fs)));
            else
                SMIN_CK(smin_pair_assemble(cur(), fp(bfv), fp(bfs), fp(bfw), ip(bank->vi), ip(bank->qi), B, i32(bfv.size(0)), i32(bfs.size(0)), Ti, Nq, D, fpm(f), fpm(fw),
                                           fpm(fs)));
        } else {
            std::tie(fw, fs) = query_encoder(st.lstm, P, query_features, st.len32, maxq, H, scoring);
            if (projection_ready) {
                await(curs, projection_ready);
                SMIN_CK(smin_video_encoder_gate(cur(), fp(st.fv), fp(fs), B, Ti, D, fpm(f)));
            } else {
                SMIN_CK(smin_video_encoder_fwd(cur(), fp(st.vx), fp(P.backbone(P_VE_W)), fp(P.backbone(P_VE_B)), fp(P.backbone(P_PE)), fp(st.vmaskf), fp(fs), B, Ti,
                                               i32(st.vx.size(2)), D, fpm(st.fv), fpm(f)));
            }
        }

        // ---- layout, part 2
        if (n_known < 0) host_wait(count_ready);
        const int64_t N = n_known < 0 ? host_n.const_data_ptr<int64_t>()[0] : n_known;
        const int n = i32(N);
        Tensor cells, row_ptr, cellmap;
        Tensor mask8 = mm.contiguous().view(at::kByte);
        hipEvent_t layout_ready;
        if (prep != curs) await(prep, count_ready);                               // (the mask; the second stream is idle while the LSTM runs)
        {
            StreamScope sc(prep);
            auto io = at::TensorOptions().dtype(at::kInt).device(dev);
            cells = at::empty({N, 4}, io); row_ptr = at::empty({Bq * L + 1}, io); cellmap = at::empty({Bq, L, L}, io);
            if (n_known < 0)
                SMIN_CK(smin_build_cells(cur(), u8(mask8), B, Li, 0, cells.data_ptr<int32_t>(), row_ptr.data_ptr<int32_t>(), cellmap.data_ptr<int32_t>()));
            else
                SMIN_CK(smin_build_cells_n(cur(), u8(mask8), B, Li, 0, n, cells.data_ptr<int32_t>(), row_ptr.data_ptr<int32_t>(), cellmap.data_ptr<int32_t>(),
                                           layout_status(dev).data_ptr<int32_t>()));
            layout_ready = mark(prep);
        }
        st.f = f; st.fw = fw; st.fs = fs; st.qmf = qmf; st.lmf = lmf; st.cells = cells; st.row_ptr = row_ptr; st.cellmap = cellmap;

        // ---- word-side operands on the second stream, behind the backbone; the main stream needs them at the first attention only
        hipEvent_t words_ready;
        wait_stream(prep, curs);
        {
            StreamScope sc(prep);
            std::vector<const float*> pp;
            for (int64_t k = 0; k < nl; ++k)
                for (int which : L_WORD_SIDE) pp.push_back(fp(P.layer(k, which)));
            st.what = at::empty({nl, B, Nq, dl}, opt); st.kb = at::empty({nl, B, Nq, dl}, opt); st.Mq = at::empty({nl, B, Nq, dl}, opt);
            st.shat = at::empty({nl, B, dl}, opt); st.uq = at::empty({nl, B, Nq}, opt);
            SMIN_CK(smin_word_prep_fwd(cur(), fp(fw), fp(fs), fp(qmf), pp.data(), i32(nl), B, Nq, D, dl, fpm(st.what), fpm(st.shat), fpm(st.kb), fpm(st.Mq), fpm(st.uq)));
            words_ready = mark(prep);
        }
        if (prep != curs) { await(curs, products_ready); await(curs, layout_ready); }
        // Tensors cross streams here without recordStream bookkeeping: DESIGN.md 6, "Stream rules" (4) says what makes that safe, for
        // scoring's early release of a layer's tensors too.

        // ---- proposal map (f_m, f_b) and every layer's clip-window term of chat
        Tensor fm = at::empty({N, D}, opt), fb = at::empty({B, L, D}, opt);
        {
            auto ws = SMIN_WS(smin_proposal_map_fwd_ws_bytes(B, Ti, D), dev);
            SMIN_CK(smin_proposal_map_fwd(cur(), fp(f), ip(cells), n, B, Ti, Li, Ci, D, nullptr, fpm(fm), fpm(fb), ws.p, ws.n));
        }
        Tensor pgs = at::empty({nl, N * C, dl}, opt);
        {
            Tensor g_all = at::empty({(int64_t)B * T, nl * dl}, opt);
            const float* xs[1] = {fp(f)};
            SMIN_CK(smin_linear_rows_fwd(cur(), xs, 1, fp(st.Wch_all), nullptr, nullptr, nullptr, 1, i32(B * T), i32(nl * dl), D, fpm(g_all)));
            auto ws = SMIN_WS(smin_clip_window_means_fwd_ws_bytes(B, Ti, dl, i32(nl)), dev);
            SMIN_CK(smin_clip_window_means_fwd(cur(), fp(g_all), fp(st.layer[0].consts), dl, ip(cells), n, B, Ti, Li, Ci, dl, i32(nl), fpm(pgs), ws.p, ws.n));
        }

        Tensor cumean = fm, Hs;                                                    // mean_c f_c of the proposal map is f_m
        // Tensors that only ever feed contractions (the pair product, the attention outputs cc_k) are stored as bf16 when the contractions
        // round their operands to bf16 anyway (smin_set_gemm_mode(2)): no bit of the step changes, half the bytes
        const bool bf16_operands = (flags & F_BF16_OPERANDS) && smin_get_gemm_mode() == 2;
        const bool cc_bf16 = bf16_operands && dl % 8 == 0;
        const bool keep_maps = (flags & F_KEEP_ATTENTION) != 0;
        TORCH_CHECK(!(scoring && keep_maps), "smin_score keeps no attention maps");
        for (int64_t k = 0; k < nl; ++k) {
            LayerState& ls = st.layer[k];
            const bool lastl = k == nl - 1;
            ls.fm = fm; ls.fb = fb;
            ls.hbar = at::empty_like(fm);
            ls.Hs = Hs;                                                            // sum of the earlier layers' gated features (undefined for k = 0)
            if (k > 0 && !lastl && N > 0) {                                        // the next layers' running sum comes out of the same pass
                Tensor Hs_next = at::empty_like(fm);
                SMIN_CK(smin_gate_fwd_sum(cur(), fp(fm), fp(fs), ip(cells), n, D, fpm(ls.hbar), fp(Hs), fpm(Hs_next)));
                Hs = Hs_next;
            } else {
                SMIN_CK(smin_gate_fwd(cur(), fp(fm), fp(fs), ip(cells), n, D, fpm(ls.hbar)));
                if (!lastl) Hs = Hs.defined() ? Hs + ls.hbar : ls.hbar;
            }
            // boundary unit on the second stream beside the content stream; joins before the moment unit
            Tensor bmap = keep_maps ? at::empty({B, L, Nq}, opt) : Tensor();       // (allocated on the main stream, written on the boundary stream)
            wait_stream(side, curs);
            {
                StreamScope sc(side);
                ls.bu = at::empty_like(fb); ls.Qb = at::empty_like(fb); ls.baq = at::empty_like(fb); ls.bqv = at::empty_like(fb); ls.Kb = at::empty_like(fw);
                ls.P = at::empty({B, L, Nq}, opt); ls.A = at::empty({B, L, L}, opt);
                SMIN_CK(smin_boundary_unit_fwd(cur(), fp(fb), fp(fw), fp(fs), fp(ls.hbar), ip(cells), ip(row_ptr), n, B, Li, Nq, D, fp(P.layer(k, L_BQ_W)), fp(P.layer(k, L_BQ_B)),
                                               fp(P.layer(k, L_BK_W)), fp(P.layer(k, L_BK_B)), fp(qmf), fp(lmf), fpm(ls.bu), fpm(ls.Qb), fpm(ls.Kb), fpm(ls.P), fpm(ls.baq),
                                               fpm(ls.bqv), fpm(ls.A)));
                if (keep_maps)                                                     // Attention.attn_weights (models.py:153) is P as written
                    TORCH_CHECK(hipMemcpyAsync(bmap.data_ptr(), ls.P.const_data_ptr(), sizeof(float) * ls.P.numel(), hipMemcpyDeviceToDevice, side.stream()) == hipSuccess,
                                "hipMemcpyAsync failed");
            }
            if (keep_maps) st.bmaps.push_back(bmap);
            // chat_k = clip-window term + [cc_0 | ..] Pcat^T + const_k + (Hs Wch^T per cell)
            Tensor chat = pgs[k];
            const Tensor& Hs_k = ls.Hs;
            for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
                Tensor hp;
                if (lo == 0) {
                    hp = at::empty({N, dl}, opt);
                    const float* xs[1] = {fp(Hs_k)};
                    SMIN_CK(smin_linear_rows_fwd(cur(), xs, 1, fp(P.layer(k, L_CH_W)), nullptr, nullptr, nullptr, 1, n, dl, D, fpm(hp)));
                }
                const int nseg = i32(std::min<int64_t>(4, k - lo));
                Tensor y = at::empty({N * C, dl}, opt);
                if (cc_bf16) {
                    const uint16_t* xh[4];
                    for (int sgm = 0; sgm < nseg; ++sgm) xh[sgm] = hp16(st.layer[lo + sgm].cc);
                    SMIN_CK(smin_linear_rows_fwd_xh(cur(), xh, nseg, fp(ls.Pcat[part]), lo == 0 ? fp(ls.consts) : nullptr, fp(chat), fp(hp), Ci, i32(N * C), dl, dl, fpm(y)));
                } else {
                    const float* xs[4];
                    for (int sgm = 0; sgm < nseg; ++sgm) xs[sgm] = fp(st.layer[lo + sgm].cc);
                    SMIN_CK(smin_linear_rows_fwd(cur(), xs, nseg, fp(ls.Pcat[part]), lo == 0 ? fp(ls.consts) : nullptr, fp(chat), fp(hp), Ci, i32(N * C), dl, dl, fpm(y)));
                }
                chat = y;
            }
            ls.chat = chat;
            if (k == 0 && prep != curs) await(curs, words_ready);
            ls.cc = at::empty({lastl ? 0 : N * C, dl}, cc_bf16 ? opt.dtype(at::kBFloat16) : opt); ls.ccmean = at::empty({N, dl}, opt);
            if (keep_maps) {                                                       // the same launch with the word probabilities stored
                Tensor probs = at::empty({N * C, (int64_t)Nq}, opt);
                SMIN_CK(smin_content_attn_fwd_probs(cur(), fp(chat), ip(cells), ip(row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]),
                                                    fp(st.shat[k]), fp(qmf), lastl ? nullptr : ls.cc.data_ptr(), cc_bf16 && !lastl ? 1 : 0, fpm(ls.ccmean), fpm(probs)));
                if (flags & F_ATTN_PACKED) {
                    st.cmaps.push_back(probs);
                } else {                                                           // ContentAttention.attn_weights in the reference's layout
                    Tensor dense = at::empty({Bq, L, L, C, (int64_t)Nq}, opt);
                    SMIN_CK(smin_content_attn_maps_dense(cur(), fp(probs), ip(cellmap), ip(cells), B, Li, Ci, dl, Nq, fp(st.uq[k]), fp(qmf), fpm(dense)));
                    st.cmaps.push_back(dense);
                }
            } else if (cc_bf16 && !lastl)
                SMIN_CK(smin_content_attn_fwd_cch(cur(), fp(chat), ip(cells), ip(row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]), fp(st.shat[k]),
                                                  fp(qmf), reinterpret_cast<uint16_t*>(ls.cc.data_ptr()), fpm(ls.ccmean)));
            else
                SMIN_CK(smin_content_attn_fwd(cur(), fp(chat), ip(cells), ip(row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]), fp(st.shat[k]), fp(qmf),
                                              lastl ? nullptr : fpm(ls.cc), fpm(ls.ccmean)));
            if (scoring && lastl) {
                // forward only: nobody but the score head reads the last mu, so the content-stream sum, the moment unit and the head
                // collapse to row dots (csrc/score_tail.hip): no cum, no x1, no mu
                wait_stream(curs, side);
                st.pm = at::empty({B, L, L}, opt); st.psea = at::empty({3, B, L}, opt);
                // (its vectors were formed with the parameter products; hbar is re-formed from fm and fs: measured faster than read)
                SMIN_CK(smin_score_tail_fwd(cur(), fp(ls.ccmean), fp(cumean), nullptr, fp(fm), fp(fs), fp(ls.bu), ip(cells), n, B, Li, D, dl, nullptr, nullptr, nullptr,
                                            nullptr, fp(P.loc(0)), nullptr, fp(st.wb), fp(bb), fp(lmf), fpm(st.pm), fpm(st.psea), st.tailv.data_ptr(),
                                            (size_t)st.tailv.numel()));
                break;
            }
            ls.cum = at::empty({N, D}, opt);
            {
                const float* xs[1] = {fp(ls.ccmean)};
                SMIN_CK(smin_linear_rows_fwd(cur(), xs, 1, fp(P.layer(k, L_C_W)), fp(P.layer(k, L_C_B)), fp(cumean), fp(ls.hbar), 1, n, D, dl, fpm(ls.cum)));
            }
            wait_stream(curs, side);
            // f_b[i] * f_b[j], kept for the weight gradient (bf16 under bf16_operands: the layer's largest saved tensor); a scorer has
            // no use for it and lets the contraction form the product as it loads (measured faster there)
            const bool x1h = bf16_operands;
            Tensor mu = at::empty_like(fm);
            if (!scoring) ls.x1 = x1h ? at::empty({N, D}, opt.dtype(at::kBFloat16)) : at::empty_like(fm);
            if (scoring) {
                SMIN_CK(smin_moment_unit_fwd(cur(), fp(ls.cum), fp(fm), fp(ls.bu), ip(cells), n, B, Li, D, fp(ls.Wcat), fp(bcat[k]), fpm(mu), nullptr));
            } else if (x1h) {
                uint16_t* xh = reinterpret_cast<uint16_t*>(ls.x1.data_ptr());
                SMIN_CK(smin_pair_product_bf16(cur(), fp(ls.bu), ip(cells), n, Li, D, xh));
                SMIN_CK(smin_moment_unit_fwd_x1h(cur(), fp(ls.cum), fp(fm), fp(ls.bu), ip(cells), n, B, Li, D, fp(ls.Wcat), fp(bcat[k]), fpm(mu), xh));
            } else {
                SMIN_CK(smin_pair_product(cur(), fp(ls.bu), ip(cells), n, Li, D, fpm(ls.x1)));
                SMIN_CK(smin_moment_unit_fwd(cur(), fp(ls.cum), fp(fm), fp(ls.bu), ip(cells), n, B, Li, D, fp(ls.Wcat), fp(bcat[k]), fpm(mu), fp(ls.x1)));
            }
            fm = mu; cumean = ls.cum; fb = ls.bu;
            if (scoring) {
                // The streams have met (the join above) and every reader of this layer's tensors is queued: all of them go except what the
                // later layers read -- its attention output cc (in `st`), mu, cum and bu (held by fm, cumean, fb), the running gate sum
                LayerState keep;
                keep.cc = ls.cc;
                ls = keep;
            }
        }
        if (scoring) return N;
        // Localization (models.py:335-344)
        Tensor pm = at::empty({B, L, L}, opt), psea = at::empty({3, B, L}, opt);
        SMIN_CK(smin_score_map_fwd(cur(), fp(fm), fp(fb), ip(cells), n, B, Li, D, fp(P.loc(0)), fp(P.loc(1)), fp(st.wb), fp(bb), fp(lmf), fpm(pm), fpm(psea)));
        st.pm = pm; st.psea = psea; st.fm_out = fm;
        return N;
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

    // The backward pass of the state run() left: the parameters' gradients in slots N_FIXED .. of the result, the inputs'
    // (F_INPUT_GRADS) in slots 0 and 1.  With the pair lists in the state (smin_forward_pairs) everything down to
    // df, dfs_parts and dfw_parts runs at batch P as it stands; smin_pair_assemble_bwd then sums the pairs onto their videos and
    // queries, and the backbone's backward runs at batch V (video encoder) and Q (sentence feature, LSTM layers).
    static variable_list backward(AutogradContext* ctx, variable_list g)
    {
        const auto [N, T, L, C, nl, flags, H, Nq_in] = SavedShape::get(ctx);
        const bool prep_kernel = (flags & F_PARAM_PREP_KERNEL) != 0;
        auto sv = ctx->get_saved_variables();
        CoreState st;
        size_state(st, nl);
        size_t cursor = 0;
        visit_state(st, [&](Tensor& t) { t = sv[cursor++]; });
        const ParamList P(std::vector<Tensor>(sv.begin() + cursor, sv.end()), nl);
        ParamList dprm(nl);                                                        // the gradients, slot for slot
        const Tensor &f = st.f, &fw = st.fw, &fs = st.fs, &qmf = st.qmf, &lmf = st.lmf, &cells = st.cells, &row_ptr = st.row_ptr, &cellmap = st.cellmap;
        const auto [dev, opt, B, D, Nq, dl, Li, Ci, Ti, curs, side] = Dims(f, f.size(0), P, T, L, C, fw.size(1), flags);
        const int n = i32(N);
        // weight-gradient contractions: nothing waits for them before the end of the step, so they go to a low-priority stream
        // of their own and fill the chip beside the bandwidth-bound kernels of the main chain
        HStream wstr = (flags & F_ASYNC_WEIGHTS) ? weight_stream(dev.index()) : curs;
        std::vector<Tensor> keep;                                                  // main-stream tensors read on wstr: alive until the streams join
        GradSync sync;
        sync.on = (flags & F_GRAD_SYNC) != 0;
        TORCH_CHECK(!sync.on || prep_kernel, "smin_forward: the in-node gradient exchange needs param_prep_kernel (SMIN._param_prep_kernel)");
        // the inputs' gradients (F_INPUT_GRADS): d video_features = the video encoder's dx, d query_features = LSTM layer 0's dX
        const bool want_dx = (flags & F_INPUT_GRADS) && ctx->needs_input_grad(0), want_dX = (flags & F_INPUT_GRADS) && ctx->needs_input_grad(1);
        TORCH_CHECK(!sync.on || !grad_sync_config().group.empty(), "smin_forward: grad_sync requested but no process group was set (smin_hip::set_grad_sync)");
        auto acc = [](Tensor& into, const Tensor& t) { if (into.defined()) into.add_(t); else into = t; };

        // ---- W^T of every contraction weight, one launch
        enum { TR_CH = 0, TR_C, TR_CAT, TR_BQ, TR_BK, TR_PER_LAYER };
        std::vector<Tensor> tr_in;
        for (int64_t k = 0; k < nl; ++k) {
            for (const Tensor& w : {P.layer(k, L_CH_W), P.layer(k, L_C_W), st.layer[k].Wcat, P.layer(k, L_BQ_W), P.layer(k, L_BK_W)}) tr_in.push_back(w);
        }
        const size_t tr_pcat0 = tr_in.size();
        for (int64_t k = 0; k < nl; ++k) for (auto& p : st.layer[k].Pcat) tr_in.push_back(p);
        const size_t tr_tail = tr_in.size();
        tr_in.push_back(st.Wch_all);
        tr_in.push_back(st.lstm[0].Wih); tr_in.push_back(st.lstm[1].Wih);
        if (want_dx) tr_in.push_back(P.backbone(P_VE_W));
        // (on the boundary stream, as the boundary heads' backward below: beside the score map's backward on the main stream, which
        //  otherwise opens the backward pass with four short launches in a row in front of the first contraction)
        HStream early = (side != curs && (flags & F_OVERLAP_PREP)) ? side : curs;
        wait_stream(early, curs);
        std::vector<Tensor> tr;
        {
            StreamScope sc(early);
            tr = transpose_all(tr_in);
        }
        auto trk = [&](int64_t k, int which) -> const Tensor& { return tr[k * TR_PER_LAYER + which]; };
        std::vector<std::vector<Tensor>> PcatT(nl);
        { size_t i = tr_pcat0; for (int64_t k = 0; k < nl; ++k) for (size_t p = 0; p < st.layer[k].Pcat.size(); ++p) PcatT[k].push_back(tr[i++]); }
        const Tensor &Wch_allT = tr[tr_tail], *WihT = &tr[tr_tail + 1];

        // ---- Localization
        const Tensor& bu_last = st.layer[nl - 1].bu;
        Tensor dpm = g[0].defined() ? cont(g[0]) : at::zeros_like(st.pm), dpsea;
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
        Tensor dfm = at::empty({N, D}, opt), dfb_next = at::empty({B, L, D}, opt);
        std::vector<Tensor> loc_bufs;
        {
            Tensor dwm = at::empty({D}, opt), dbm = at::empty({1}, opt), dwb = at::empty({3, D}, opt), dbb = at::empty({3}, opt);
            if (early != curs) {
                wait_stream(early, curs);                                          // (behind the allocations above: "Stream rules" (2))
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
                await(curs, early_done);                                           // W^T and dfb_next
            } else {
                auto ws = SMIN_WS(smin_score_map_bwd_ws_bytes(n, B, Li, D), dev);
                SMIN_CK(smin_score_map_bwd(cur(), fp(dpm), fp(dpsea), fp(st.pm), fp(st.psea), fp(st.fm_out), fp(bu_last), ip(cells), n, B, Li, D, fp(P.loc(0)), fp(st.wb), fp(lmf),
                                           fpm(dfm), fpm(dfb_next), fpm(dwm), fpm(dbm), fpm(dwb), fpm(dbb), ws.p, ws.n));
            }
            loc_bufs = {dwm, dbm, dwb, dbb};
            dprm.loc(0) = dwm.view_as(P.loc(0)); dprm.loc(1) = dbm.view_as(P.loc(1));
            for (int h = 0; h < 3; ++h) { dprm.loc(2 + 2 * h) = dwb[h].view_as(P.loc(2 + 2 * h)); dprm.loc(3 + 2 * h) = dbb.slice(0, h, h + 1).view_as(P.loc(3 + 2 * h)); }
        }

        std::vector<Tensor> dcc(nl), dHs(nl), dchat(nl), dconsts(nl), dfs_parts, dfw_parts;
        // prep_kernel: the gradients that meet in the parameter products are gathered as the kernel of csrc/param_prep.hip wants them
        Tensor dconsts_all, dWcat_all, dbcat_all, dWch_all;
        std::vector<Tensor> base_ch(nl), base_c(nl), base_bc(nl);
        if (prep_kernel) {
            dconsts_all = at::empty({nl, dl}, opt); dWcat_all = at::empty({nl, D, 2 * D}, opt); dbcat_all = at::empty({nl, D}, opt);
            for (int64_t k = 0; k < nl; ++k) dconsts[k] = dconsts_all[k];
        }
        std::vector<std::vector<Tensor>> dPcat(nl);
        Tensor dwhat = at::empty_like(st.what), dshat = at::empty_like(st.shat), dMq = at::empty_like(st.Mq), duq = at::empty_like(st.uq);
        if (N == 0) { dwhat.zero_(); dshat.zero_(); dMq.zero_(); duq.zero_(); }
        Tensor dcum_next;                                                          // gradient of cum_k from layer k+1's clip-mean chain
        hipEvent_t attn0_done = nullptr;
        hipEvent_t boundary_done = nullptr;                                        // the previous iteration's boundary-unit backward (side stream)
        for (int64_t k = nl - 1; k >= 0; --k) {
            LayerState& ls = st.layer[k];
            // moment unit: dmu -> d cum (its chain gradient folded in), d bu, weight gradients; the residual gradient is dmu itself
            Tensor dcum = at::empty({N, D}, opt), dfb_mu = at::empty({B, L, D}, opt);
            keep.push_back(dfm); keep.push_back(dcum);
            // (measured: the weight half queued ahead of the input half 21.39 -> 21.15 ms/step, behind it 21.7 -> 21.6)
            {
                wait_stream(wstr, curs);
                StreamScope sc(wstr);
                Tensor dWcat = prep_kernel ? dWcat_all[k] : at::empty_like(ls.Wcat), dbcat = prep_kernel ? dbcat_all[k] : at::empty({D}, opt);
                auto ws = SMIN_WS(smin_moment_unit_bwd_ws_bytes(n, B, Li, D), dev);
                if (ls.x1.scalar_type() == at::kBFloat16)
                    SMIN_CK(smin_moment_unit_bwd_x1h(cur(), fp(dfm), fp(ls.cum), fp(ls.bu), ip(cells), ip(row_ptr), ip(cellmap), n, B, Li, D, fp(trk(k, TR_CAT)), nullptr, nullptr,
                                                     fpm(dWcat), fpm(dbcat), ws.p, ws.n, 1, nullptr, reinterpret_cast<const uint16_t*>(ls.x1.const_data_ptr()), nullptr));
                else
                    SMIN_CK(smin_moment_unit_bwd(cur(), fp(dfm), fp(ls.cum), fp(ls.bu), ip(cells), ip(row_ptr), ip(cellmap), n, B, Li, D, fp(trk(k, TR_CAT)), nullptr, nullptr,
                                                 fpm(dWcat), fpm(dbcat), ws.p, ws.n, 1, nullptr, fp(ls.x1), nullptr));
                if (!prep_kernel) {
                    dprm.layer(k, L_FB_W) = dWcat.slice(1, 0, D).contiguous().view_as(P.layer(k, L_FB_W));
                    dprm.layer(k, L_FC_W) = dWcat.slice(1, D).contiguous().view_as(P.layer(k, L_FC_W));
                    dprm.layer(k, L_FB_B) = dbcat; dprm.layer(k, L_FC_B) = dbcat;
                }
                sync.reduce({dWcat, dbcat}, wstr);                                   // inputs of the parameter-product kernel
            }
            // the previous layer's boundary-unit backward (second stream) is awaited HERE, where its dfb is first read -- not in front of
            // that layer's gate backward, which reads nothing of it any more (it forms the unit's dhbar itself): the main stream sat
            // ~0.6 ms behind the unit's weight contractions at the end of layer 0 (tools/gantt.sh)
            if (boundary_done) { await(curs, boundary_done); boundary_done = nullptr; }
            {
                auto ws = SMIN_WS(smin_moment_unit_bwd_ws_bytes(n, B, Li, D), dev);
                SMIN_CK(smin_moment_unit_bwd(cur(), fp(dfm), fp(ls.cum), fp(ls.bu), ip(cells), ip(row_ptr), ip(cellmap), n, B, Li, D, fp(trk(k, TR_CAT)), fpm(dcum), fpm(dfb_mu),
                                             nullptr, nullptr, ws.p, ws.n, 1, fp(dcum_next), nullptr, fp(dfb_next)));   // (the pair product feeds the weight half only)
            }                                                                      // dfb_mu = this unit's gradient of bu + the later consumer's (dfb_next): dbu
            // boundary unit on the second stream
            // (the boundary unit's gradient of hbar, A[b,i,j] * dbu[b,i,:], is formed by the gate backward itself from A and dbu: no [N][D]
            //  tensor written here and read back there)
            Tensor dfb_k, dbu;
            wait_stream(side, curs);
            {
                StreamScope sc(side);
                dbu = dfb_mu;
                dfb_k = at::empty({B, L, D}, opt);
                Tensor dfw = at::empty_like(fw), dfs = at::empty_like(fs);
                Tensor dWq = at::empty({D, D}, opt), dbq = at::empty({D}, opt), dWk = at::empty({D, D}, opt), dbk = at::empty({D}, opt);
                auto ws = SMIN_WS(smin_boundary_unit_bwd_ws_bytes(B, Li, Nq, D), dev);
                SMIN_CK(smin_boundary_unit_bwd(cur(), fp(dbu), fp(ls.fb), fp(fw), fp(fs), fp(ls.hbar), ip(cells), ip(row_ptr), n, B, Li, Nq, D, fp(trk(k, TR_BQ)), fp(trk(k, TR_BK)),
                                               fp(qmf), fp(lmf), fp(ls.Qb), fp(ls.Kb), fp(ls.P), fp(ls.baq), fp(ls.bqv), fp(ls.A), fpm(dfb_k), fpm(dfw), fpm(dfs), nullptr,
                                               fpm(dWq), fpm(dbq), fpm(dWk), fpm(dbk), ws.p, ws.n));
                dprm.layer(k, L_BQ_W) = dWq; dprm.layer(k, L_BQ_B) = dbq; dprm.layer(k, L_BK_W) = dWk; dprm.layer(k, L_BK_B) = dbk;
                sync.reduce({dWq, dbq, dWk, dbk}, side);
                dfs_parts.push_back(dfs); dfw_parts.push_back(dfw);
                keep.push_back(dfb_next); keep.push_back(dfb_mu); keep.push_back(dbu);
            }
            if (side != curs) boundary_done = mark(side);
            // clip-mean update cum = ccmean Wc^T + b + cumean + hbar: d ccmean, weight gradients; d cumean = d hbar = dcum
            Tensor dccmean = at::empty({N, dl}, opt);
            {
                const float* xs[1] = {fp(ls.ccmean)}; float* dxs[1] = {fpm(dccmean)};
                auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, D, dl), dev);
                SMIN_CK(smin_linear_rows_bwd(cur(), fp(dcum), xs, 1, fp(trk(k, TR_C)), n, D, dl, dxs, nullptr, nullptr, ws.p, ws.n));
            }
            // attention core
            dchat[k] = at::empty({N * C, dl}, opt);
            if (N > 0) {
                auto ws = scratch(smin_content_attn_bwd_workspace_bytes(n, B, Ci, dl), dev);
                SMIN_CK(smin_content_attn_bwd(cur(), fp(dcc[k]), fp(dccmean), fp(ls.chat), ip(cells), ip(row_ptr), n, B, Li, Ci, dl, Nq, fp(st.Mq[k]), fp(st.uq[k]), fp(st.what[k]),
                                              fp(st.shat[k]), fp(qmf), fpm(dchat[k]), fpm(dMq[k]), fpm(duq[k]), fpm(dwhat[k]), fpm(dshat[k]), ws.p, ws.n));
            }
            if (k == 0) attn0_done = mark(curs);                                // every dchat / word-side gradient is final from here on
            // chat_k's contraction over the earlier layers' attention outputs, and its per-cell gate term: input gradients
            Tensor dhp;
            for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
                const int nseg = i32(std::min<int64_t>(4, k - lo));
                const float* xs[4]; float* dxs[4];
                // every earlier layer's attention output already has the gradient of the later layers (all of them, or none for the last
                // layer): accumulate in the epilogue instead of a full-size add per tensor afterwards
                const bool have = dcc[lo].defined();
                for (int sgm = 0; sgm < nseg; ++sgm) {
                    TORCH_CHECK(dcc[lo + sgm].defined() == have, "content stream: inconsistent gradient state of the attention outputs");
                    xs[sgm] = nullptr;                                             // (the input gradients never read the operands)
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
                dhp = at::empty({N, dl}, opt);
                keep.push_back(dhp);
                SMIN_CK(smin_group_sum(cur(), fp(dchat[k]), n, Ci, dl, fpm(dhp)));
                dHs[k] = at::empty({N, D}, opt);
                const float* xs[1] = {fp(ls.Hs)}; float* dxs[1] = {fpm(dHs[k])};
                auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, dl, D), dev);
                SMIN_CK(smin_linear_rows_bwd(cur(), fp(dhp), xs, 1, fp(trk(k, TR_CH)), n, dl, D, dxs, nullptr, nullptr, ws.p, ws.n));
            }
            // ... and this layer's weight gradients of the content stream
            wait_stream(wstr, curs);
            {
                StreamScope sc(wstr);
                {
                    Tensor dWc = at::empty_like(P.layer(k, L_C_W)), dbc = at::empty({D}, opt);
                    const float* xs[1] = {fp(ls.ccmean)};
                    auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, D, dl), dev);
                    SMIN_CK(smin_linear_rows_bwd(cur(), fp(dcum), xs, 1, nullptr, n, D, dl, nullptr, fpm(dWc), fpm(dbc), ws.p, ws.n));
                    if (prep_kernel) { base_c[k] = dWc; base_bc[k] = dbc; }
                    else { acc(dprm.layer(k, L_C_W), dWc); acc(dprm.layer(k, L_C_B), dbc); }
                }
                for (int64_t part = 0, lo = 0; lo < k; ++part, lo += 4) {
                    const int nseg = i32(std::min<int64_t>(4, k - lo));
                    Tensor dP = at::empty_like(ls.Pcat[part]);
                    if (lo == 0 && !prep_kernel) dconsts[k] = at::empty({dl}, opt);
                    auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(i32(N * C), dl, nseg * dl), dev);
                    if (st.layer[lo].cc.scalar_type() == at::kBFloat16) {
                        const uint16_t* xh[4];
                        for (int sgm = 0; sgm < nseg; ++sgm) xh[sgm] = hp16(st.layer[lo + sgm].cc);
                        SMIN_CK(smin_linear_rows_bwd_xh(cur(), fp(dchat[k]), xh, nseg, i32(N * C), dl, dl, fpm(dP), lo == 0 ? fpm(dconsts[k]) : nullptr, ws.p, ws.n));
                    } else {
                        const float* xs[4];
                        for (int sgm = 0; sgm < nseg; ++sgm) xs[sgm] = fp(st.layer[lo + sgm].cc);
                        SMIN_CK(smin_linear_rows_bwd(cur(), fp(dchat[k]), xs, nseg, nullptr, i32(N * C), dl, dl, nullptr, fpm(dP), lo == 0 ? fpm(dconsts[k]) : nullptr, ws.p, ws.n));
                    }
                    dPcat[k].push_back(dP);
                }
                if (k > 0) {
                    Tensor dWch = at::empty_like(P.layer(k, L_CH_W));
                    const float* xs[1] = {fp(ls.Hs)};
                    auto ws = scratch(smin_linear_rows_bwd_workspace_bytes(n, dl, D), dev);
                    SMIN_CK(smin_linear_rows_bwd(cur(), fp(dhp), xs, 1, nullptr, n, dl, D, nullptr, fpm(dWch), nullptr, ws.p, ws.n));
                    if (prep_kernel) base_ch[k] = dWch; else acc(dprm.layer(k, L_CH_W), dWch);
                }
            }
            // gate: every consumer of hbar_k (clip-mean update, boundary unit, the later layers' running sums) and of f_m (residual; layer 0: the clip-mean chain)
            {
                std::vector<Tensor> later;
                for (int64_t kk = k + 1; kk < nl; ++kk) later.push_back(dHs[kk]);
                std::vector<const float*> dh{fp(dcum)}, dr{fp(dfm)};
                Tensor later_sum;
                if (later.size() <= 3) for (auto& t : later) dh.push_back(fp(t));
                else { later_sum = sum_list(later); dh.push_back(fp(later_sum)); }
                if (k == 0) dr.push_back(fp(dcum));
                Tensor dfm_k = at::empty({N, D}, opt), dfs = at::empty_like(fs);
                auto ws = SMIN_WS(smin_gate_bwd_ws_bytes(B, Li, D), dev);
                SMIN_CK(smin_gate_bwd(cur(), dh.data(), i32(dh.size()), dr.data(), i32(dr.size()), fp(ls.fm), fp(fs), ip(row_ptr), n, B, Li, D, fpm(dfm_k), fpm(dfs), ws.p, ws.n,
                                      ip(cells), fp(ls.A), fp(dbu)));
                dfs_parts.push_back(dfs);
                dfm = dfm_k;
            }
            dcum_next = dcum; dfb_next = dfb_k;
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
        hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
        TORCH_CHECK(hipStreamIsCapturing(curs.stream(), &capture) == hipSuccess, "hipStreamIsCapturing failed");
        const bool tail_split = (flags & F_TAIL_SPLIT) && capture == hipStreamCaptureStatusNone;
        HStream tail = (flags & F_OVERLAP_PREP) ? side_stream(dev.index()) : curs;
        HStream wordst = !(flags & F_OVERLAP_PREP) ? curs : tail_split ? side_stream(dev.index(), 1) : tail;
        HStream cw = tail_split ? tail : curs;                                      // stream of the clip-window gradients
        if (!attn0_done) attn0_done = mark(curs);
        hipEvent_t words_done;
        if (!tail_split) wait_stream(wordst, curs);
        else if (wordst != curs) await(wordst, attn0_done);
        {
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
        Tensor df;
        hipEvent_t weights_done;
        bool tab_built = false;
        auto tab = clip_event_table(dev, Ti, Li, Ci, &tab_built);
        if (tab_built) wait_stream(cw, curs);                                    // first backward of this geometry only ("Stream rules" (1))
        {
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
                const float* xs[1] = {fp(f)};
                dWch_all = at::empty_like(st.Wch_all);
                auto wsw = scratch(smin_linear_rows_bwd_workspace_bytes(i32(B * T), i32(nl * dl), D), dev);
                SMIN_CK(smin_linear_rows_bwd(cur(), fp(dg), xs, 1, nullptr, i32(B * T), i32(nl * dl), D, nullptr, fpm(dWch_all), nullptr, wsw.p, wsw.n));
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
            SMIN_CK(smin_linear_rows_dx_acc(cur(), fp(dg), 1, fp(Wch_allT), i32(B * T), i32(nl * dl), D, dxs));
        }

        // ---- parameter products on the second stream: consts_k = b_ch_k + Wch_k bsum_k (bsum_k = sum_{l<k} b_c_l), Pcat_k = [Wch_k Wc_l]_l
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
        if (prep_kernel) {
            StreamScope sc(tail);
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
        } else {
            StreamScope sc(tail);
            Tensor bsum;
            std::vector<Tensor> bsums(nl);
            for (int64_t k = 0; k < nl; ++k) { bsums[k] = bsum; bsum = bsum.defined() ? bsum + P.layer(k, L_C_B) : P.layer(k, L_C_B); }
            Tensor dbsum_run;                                                       // sum_{k' > l} Wch_k'^T dconst_k'
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

        // ---- backbone on the main stream: video encoder, sentence / word features, the two LSTM layers (models.py:38-83)
        std::vector<Tensor> lstm_bufs;
        Tensor dvideo, dquery;
        // the backbone's weight halves: on the word stream (idle by now) when there is one -- the weight stream still holds layer 0's
        // moment-unit contraction, and these short kernels close the step
        HStream bstr = (tail_split && wordst != curs && wstr != curs) ? wordst : wstr;
        {
            const int Din = i32(st.vx.size(2));
            const int64_t pe_rows = P.backbone(P_PE).size(0);
            const bool pairs = st.vi.defined();
            const int Bv = i32(st.vx.size(0)), Bw = i32(st.lstm[0].x.size(0));     // rows of the video encoder and of the query encoder (B unless pairs)
            Tensor dfs_video = at::empty({(int64_t)Bv, (int64_t)D}, opt);
            dprm.backbone(P_VE_W) = at::empty({D, Din}, opt); dprm.backbone(P_VE_B) = at::empty({D}, opt);
            dprm.backbone(P_PE) = pe_rows != T ? at::zeros({pe_rows, D}, opt) : at::empty({T, D}, opt);
            // every call below is split into its inputs half (main stream, the dependent chain) and its weights half (weight stream); the
            // intermediate of a pair lives in a buffer of its own (the per-stream scratch is reused by the next call on that stream)
            auto own = [&](size_t nbytes) {
                Tensor t = at::empty({(int64_t)nbytes + 256}, at::TensorOptions().dtype(at::kByte).device(dev));
                keep.push_back(t);
                return t;
            };
            Tensor wsv = own(smin_video_encoder_bwd_workspace_bytes(Bv, Ti, Din, D));
            Tensor dfs_total, dfw_total, venc_fs = fs;
            if (pairs) {
                // the pairs' gradients onto their videos and queries (csrc/corpus.hip): df -> dfv, the per-pair sums of dfw / dfs and the
                // product's gradient of f_s -> the query bank's rows.  The video encoder's backward has no fs == NULL mode: it takes dfv as
                // its df and ones as fs (a multiplication by 1.0f is exact; its dfs output is not used).
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
            SMIN_CK(smin_video_encoder_bwd(cur(), fp(df), fp(st.fv), fp(venc_fs), fp(st.vmaskf), fp(st.vx), Bv, Ti, Din, D, nullptr, nullptr, nullptr, fpm(dfs_video),
                                           wsv.data_ptr(), (size_t)wsv.numel()));
            if (!pairs) {
                dfs_parts.push_back(dfs_video);
                if (wordst != curs) await(curs, words_done);
                dfs_total = sum_list(dfs_parts); dfw_total = sum_list(dfw_parts);
            }
            // f_s = [f_w[b, len_b - 1, :H] | f_w[b, 0, H:]] (models.py:60-62)
            SMIN_CK(smin_sentence_feature_bwd(cur(), fp(dfs_total), ip(st.len32), Bw, Nq, i32(H), fpm(dfw_total)));
            Tensor dH = Nq_in < Nq ? dfw_total.slice(1, 0, Nq_in).contiguous() : dfw_total;
            keep.push_back(dfs_total); keep.push_back(dfw_total); keep.push_back(dH); keep.push_back(df); keep.push_back(dfs_video);
            wait_stream(bstr, curs);
            {
                StreamScope sc(bstr);
                SMIN_CK(smin_video_encoder_bwd(cur(), nullptr, fp(st.fv), fp(venc_fs), fp(st.vmaskf), fp(st.vx), Bv, Ti, Din, D, fpm(dprm.backbone(P_VE_W)), fpm(dprm.backbone(P_VE_B)),
                                               fpm(dprm.backbone(P_PE)), nullptr, wsv.data_ptr(), (size_t)wsv.numel()));
            }
            for (int layer = 1; layer >= 0; --layer) {
                LstmState& ls = st.lstm[layer];
                const int In = i32(ls.x.size(2)), Hh = i32(H);
                Tensor dX = layer > 0 || want_dX ? at::empty_like(ls.x) : Tensor();
                Tensor dWih = at::empty_like(ls.Wih), dbias = at::empty({8 * H}, opt), dWhh = at::empty_like(ls.Whh);
                lstm_bufs.push_back(dWih); lstm_bufs.push_back(dbias); lstm_bufs.push_back(dWhh);
                Tensor wsl = own(smin_bilstm_layer_bwd_workspace_bytes(Bw, i32(Nq_in), In, Hh));
                SMIN_CK(smin_bilstm_layer_bwd(cur(), fp(dH), fp(ls.x), fp(ls.Hout), fp(ls.G), fp(ls.Cs), fp(WihT[layer]), fp(ls.Whh), ip(st.len32), Bw, i32(Nq_in), In, Hh,
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
            dquery = dH;
            // the video features' gradient behind the last recurrence, on the main stream: the cluster recurrences need every CU's LDS
            // co-resident, and here only the layer-0 weight pieces are left beside it (measured against the weight stream: DESIGN 6)
            if (want_dx) {
                dvideo = at::empty_like(st.vx);
                SMIN_CK(smin_video_encoder_bwd_input(cur(), fp(tr[tr_tail + 3]), fp(st.vmaskf), Bv, Ti, Din, D, fpm(dvideo), wsv.data_ptr(), (size_t)wsv.numel()));
            }
        }
        wait_stream(curs, tail);
        wait_stream(curs, wstr);
        wait_stream(curs, wordst);
        if (sync.on) {
            std::vector<Tensor> late{dprm.backbone(P_VE_W), dprm.backbone(P_VE_B), dprm.backbone(P_PE)};
            for (auto& t : lstm_bufs) late.push_back(t);
            sync.reduce(late, curs);
            sync.join(curs);
        }

        variable_list out(N_FIXED + dprm.all.size());
        if (want_dx) out[0] = dvideo;
        if (want_dX) out[1] = dquery;
        std::copy(dprm.all.begin(), dprm.all.end(), out.begin() + N_FIXED);
        return out;
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

// training.pair_rank_loss: the contrastive term over a pair plan's P pairs (see PairRankNode above); gradients to pm, ps, pe only
std::tuple<Tensor, Tensor, Tensor> smin_pair_rank_loss(const Tensor& pm, const Tensor& ps, const Tensor& pe, const Tensor& moment_mask, const Tensor& q_ptr,
                                                       const Tensor& q_pairs, const Tensor& positive, double tau, double gamma)
{
    for (const Tensor* t : {&pm, &ps, &pe, &moment_mask, &q_ptr, &q_pairs, &positive})
        TORCH_CHECK(t->is_cuda(), "smin_pair_rank_loss runs on a HIP device only (there is no CPU fallback)");
    for (const Tensor* t : {&ps, &pe, &moment_mask, &q_ptr, &q_pairs, &positive})
        TORCH_CHECK(t->device() == pm.device(), "smin_pair_rank_loss: every tensor on one device");
    const int64_t P = pm.dim() == 3 ? pm.size(0) : -1, L = pm.dim() == 3 ? pm.size(1) : -1;
    TORCH_CHECK(P >= 1 && L >= 1 && pm.size(2) == L && ps.sizes() == at::IntArrayRef({P, L}) && pe.sizes() == ps.sizes() && moment_mask.sizes() == pm.sizes(),
                "smin_pair_rank_loss: pm (P, L, L), ps (P, L), pe (P, L) and moment_mask (P, L, L) with P, L >= 1");
    TORCH_CHECK(q_ptr.dim() == 1 && q_ptr.size(0) >= 2 && q_pairs.dim() == 1 && q_pairs.size(0) == P && positive.dim() == 1 && positive.size(0) == P,
                "smin_pair_rank_loss: q_ptr (Q + 1,) with Q >= 1, q_pairs (P,) and positive (P,)");
    TORCH_CHECK(std::isfinite(tau) && tau > 0 && std::isfinite(gamma) && gamma > 0, "smin_pair_rank_loss: tau and gamma must be finite and positive");
    c10::hip::HIPGuard device_guard(pm.device().index());
    auto out = PairRankNode::apply(pm, ps, pe, moment_mask, q_ptr, q_pairs, positive, tau, gamma);
    return std::make_tuple(out[0], out[1], out[2]);
}

// training.pair_distill_loss: the soft-target term over a pair plan's P pairs (see PairDistillNode above); gradients to pm, ps, pe only
std::tuple<Tensor, Tensor, Tensor> smin_pair_distill_loss(const Tensor& pm, const Tensor& ps, const Tensor& pe, const Tensor& moment_mask, const Tensor& q_ptr,
                                                          const Tensor& q_pairs, const Tensor& teacher, double tau, double gamma, double gamma_teacher)
{
    for (const Tensor* t : {&pm, &ps, &pe, &moment_mask, &q_ptr, &q_pairs, &teacher})
        TORCH_CHECK(t->is_cuda(), "smin_pair_distill_loss runs on a HIP device only (there is no CPU fallback)");
    for (const Tensor* t : {&ps, &pe, &moment_mask, &q_ptr, &q_pairs, &teacher})
        TORCH_CHECK(t->device() == pm.device(), "smin_pair_distill_loss: every tensor on one device");
    const int64_t P = pm.dim() == 3 ? pm.size(0) : -1, L = pm.dim() == 3 ? pm.size(1) : -1;
    TORCH_CHECK(P >= 1 && L >= 1 && pm.size(2) == L && ps.sizes() == at::IntArrayRef({P, L}) && pe.sizes() == ps.sizes() && moment_mask.sizes() == pm.sizes(),
                "smin_pair_distill_loss: pm (P, L, L), ps (P, L), pe (P, L) and moment_mask (P, L, L) with P, L >= 1");
    TORCH_CHECK(q_ptr.dim() == 1 && q_ptr.size(0) >= 2 && q_pairs.dim() == 1 && q_pairs.size(0) == P && teacher.dim() == 1 && teacher.size(0) == P,
                "smin_pair_distill_loss: q_ptr (Q + 1,) with Q >= 1, q_pairs (P,) and teacher (P,)");
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
