// Host-side plumbing of the torch extension (torch_binding.cpp): pointer and dtype helpers, stream scopes, events and the two
// hand-off verbs, the side streams, per-stream scratch, the in-node gradient exchange, the parameter list, batched transposes and sums.
#pragma once
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

// ---------------------------------------------------------------- operand-dtype twins
// A tensor that only feeds contractions is stored as fp32 or, under bf16_operand_storage, as bf16, and the C ABI has an
// entry point per storage.  One function per family: it reads the dtype of the tensor it is handed and calls the fp32 entry point or
// its bf16 twin on the current stream, with the arguments in the entry point's own order.
inline bool is_bf16(const Tensor& t) { return t.defined() && t.scalar_type() == at::kBFloat16; }

// smin_linear_rows_fwd over `nseg` <= 4 row operands of one storage
void linear_rows_fwd(const Tensor* const* xs, int nseg, const float* W, const float* bias, const float* add_rows, const float* add_cells, int C, int R, int O, int K,
                     float* y)
{
    if (is_bf16(*xs[0])) {
        const uint16_t* xh[4];
        for (int s = 0; s < nseg; ++s) xh[s] = hp16(*xs[s]);
        SMIN_CK(smin_linear_rows_fwd_xh(cur(), xh, nseg, W, bias, add_rows, add_cells, C, R, O, K, y));
    } else {
        const float* xf[4];
        for (int s = 0; s < nseg; ++s) xf[s] = fp(*xs[s]);
        SMIN_CK(smin_linear_rows_fwd(cur(), xf, nseg, W, bias, add_rows, add_cells, C, R, O, K, y));
    }
}
// the weights half of smin_linear_rows_bwd over the same operands
void linear_rows_bwd_weights(const float* dy, const Tensor* const* xs, int nseg, int R, int O, int K, float* dW, float* dbias, const Scratch& ws)
{
    if (is_bf16(*xs[0])) {
        const uint16_t* xh[4];
        for (int s = 0; s < nseg; ++s) xh[s] = hp16(*xs[s]);
        SMIN_CK(smin_linear_rows_bwd_xh(cur(), dy, xh, nseg, R, O, K, dW, dbias, ws.p, ws.n));
    } else {
        const float* xf[4];
        for (int s = 0; s < nseg; ++s) xf[s] = fp(*xs[s]);
        SMIN_CK(smin_linear_rows_bwd(cur(), dy, xf, nseg, nullptr, R, O, K, nullptr, dW, dbias, ws.p, ws.n));
    }
}
// The moment unit's forward.  x1 allocated: the pair product f_b[i] * f_b[j] is formed into it first, in its storage, and kept for the
// weight gradient; x1 undefined (a scorer): the contraction forms the product as it loads.
void moment_unit_fwd(const float* cum, const float* fm, const float* bu, const int32_t* cells, int n, int B, int L, int D, const float* Wcat, const float* bcat,
                     float* mu, const Tensor& x1)
{
    if (is_bf16(x1)) {
        uint16_t* xh = reinterpret_cast<uint16_t*>(x1.data_ptr());
        SMIN_CK(smin_pair_product_bf16(cur(), bu, cells, n, L, D, xh));
        SMIN_CK(smin_moment_unit_fwd_x1h(cur(), cum, fm, bu, cells, n, B, L, D, Wcat, bcat, mu, xh));
    } else {
        if (x1.defined()) SMIN_CK(smin_pair_product(cur(), bu, cells, n, L, D, fpm(x1)));
        SMIN_CK(smin_moment_unit_fwd(cur(), cum, fm, bu, cells, n, B, L, D, Wcat, bcat, mu, fp(x1)));
    }
}
// smin_moment_unit_bwd (all_valid = 1) with the saved pair product in its storage; x1 undefined: the input half, which does not read it
void moment_unit_bwd(const float* dmu, const float* cum, const float* bu, const int32_t* cells, const int32_t* row_ptr, const int32_t* cellmap, int n, int B, int L,
                     int D, const float* WcatT, float* dcum, float* dfb, float* dWcat, float* dbcat, const Scratch& ws, const float* dcum_acc, const Tensor& x1,
                     const float* dfb_acc)
{
    if (is_bf16(x1))
        SMIN_CK(smin_moment_unit_bwd_x1h(cur(), dmu, cum, bu, cells, row_ptr, cellmap, n, B, L, D, WcatT, dcum, dfb, dWcat, dbcat, ws.p, ws.n, 1, dcum_acc, hp16(x1), dfb_acc));
    else
        SMIN_CK(smin_moment_unit_bwd(cur(), dmu, cum, bu, cells, row_ptr, cellmap, n, B, L, D, WcatT, dcum, dfb, dWcat, dbcat, ws.p, ws.n, 1, dcum_acc, fp(x1), dfb_acc));
}
// The content-attention core.  cc: the attention rows in their storage, or undefined (the last layer keeps none); probs: the word
// probabilities of every packed row when the maps are kept, else undefined.
void content_attn_fwd(const float* chat, const int32_t* cells, const int32_t* row_ptr, int n, int B, int L, int C, int dl, int Nq, const float* Mq, const float* uq,
                      const float* what, const float* shat, const float* qmask, const Tensor& cc, float* ccmean, const Tensor& probs)
{
    if (probs.defined())                                                       // the same launch with the word probabilities stored
        SMIN_CK(smin_content_attn_fwd_probs(cur(), chat, cells, row_ptr, n, B, L, C, dl, Nq, Mq, uq, what, shat, qmask, cc.defined() ? cc.data_ptr() : nullptr,
                                            is_bf16(cc) ? 1 : 0, ccmean, fpm(probs)));
    else if (is_bf16(cc))
        SMIN_CK(smin_content_attn_fwd_cch(cur(), chat, cells, row_ptr, n, B, L, C, dl, Nq, Mq, uq, what, shat, qmask, reinterpret_cast<uint16_t*>(cc.data_ptr()), ccmean));
    else
        SMIN_CK(smin_content_attn_fwd(cur(), chat, cells, row_ptr, n, B, L, C, dl, Nq, Mq, uq, what, shat, qmask, fpm(cc), ccmean));
}

}  // namespace
