// R@n, IoU=m metric of the reference (utils.py:10-31) on the device:
//   score = pm * sqrt(ps[i]) * sqrt(pe[j]) * moment_mask ; top-5 moments per sample ; hit if any of the top-n has IoU > m.
// One workgroup per sample: per-thread running top-5 over the streamed scores, then five rounds of block arg-max over the
// candidates (ties -> lowest flat index; torch.topk leaves tie order unspecified, so ties are "parity unpinned"), then the
// 2 x 4 hit flags; a second pass sums the samples.  One host read per call.  No limit on L.
//
// The epoch meter (smin_epoch_meter_update, include/smin_hip.h) runs the same per-sample stage -- this file's for the reference's
// rule, moments.hip's for the NMS rule -- and closes with one wave that adds the batch's sums to an fp64 accumulator in device
// memory: no host read per batch, no atomics, the order of every sum fixed.
#include "common.h"
#include "smin_hip.h"

namespace smin {

// candidate order of the metric: higher score first, ties -> lower flat index
__device__ __forceinline__ bool better(float v, int k, float bv, int bi) { return v > bv || (v == bv && k < bi); }

__global__ __launch_bounds__(256)
void ious_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe, const uint8_t* __restrict__ mm,
                 const float* __restrict__ sm, int L, float* __restrict__ hits /* [B][8] */, float* __restrict__ top1 /* [B] or null */)
{
    // Any L: each thread streams its share of the L*L scores keeping its own five best in registers (no score buffer, so
    // the 512 x 512 long-video map costs the same LDS as a 16 x 16 one); the 256 x 5 candidates then go through five rounds
    // of workgroup arg-max.
    __shared__ float cv[256 * 5];
    __shared__ int ci[256 * 5];
    __shared__ float rv[4];
    __shared__ int ri[4], rs[4];
    __shared__ float top[5];
    const int b = blockIdx.x, t = threadIdx.x, n = L * L;
    float v5[5]; int i5[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) { v5[r] = -INFINITY; i5[r] = 0x7fffffff; }
    const float* psb = ps + (size_t)b * L;
    const float* peb = pe + (size_t)b * L;
    for (int k = t; k < n; k += 256) {
        const int i = k / L, j = k - i * L;
        const size_t o = (size_t)b * n + k;
        float v = pm[o] * sqrtf(psb[i]) * sqrtf(peb[j]) * (mm[o] ? 1.f : 0.f);
        int kk = k;
        if (better(v, kk, v5[4], i5[4])) {
#pragma unroll
            for (int r = 0; r < 5; ++r) {               // insertion into the sorted five
                if (better(v, kk, v5[r], i5[r])) { const float tv = v5[r]; const int ti = i5[r]; v5[r] = v; i5[r] = kk; v = tv; kk = ti; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) { cv[t * 5 + r] = v5[r]; ci[t * 5 + r] = i5[r]; }
    __syncthreads();
    for (int r = 0; r < 5; ++r) {
        float bv = -INFINITY; int bi = 0x7fffffff, bs = 0;
        for (int s = t; s < 256 * 5; s += 256) { if (better(cv[s], ci[s], bv, bi)) { bv = cv[s]; bi = ci[s]; bs = s; } }
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o); const int os = __shfl_xor(bs, o);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; bs = os; }
        }
        if ((t & 63) == 0) { rv[t >> 6] = bv; ri[t >> 6] = bi; rs[t >> 6] = bs; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < 4; ++w) if (better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; bs = rs[w]; }
            top[r] = (bi < n) ? sm[(size_t)b * n + bi] : 0.f;
            if (bi < n) { cv[bs] = -INFINITY; ci[bs] = 0x7fffffff; }
        }
        __syncthreads();
    }
    if (t < 8) {
        const int nn = t < 4 ? 1 : 5;
        const float thr = (t & 3) == 0 ? 0.1f : (t & 3) == 1 ? 0.3f : (t & 3) == 2 ? 0.5f : 0.7f;
        bool hit = false;
        for (int r = 0; r < nn; ++r) hit = hit || top[r] > thr;
        hits[(size_t)b * 8 + t] = hit ? 1.f : 0.f;
    }
    if (t == 0 && top1) top1[b] = top[0];                       // the meter's top-1 IoU: sm at the best cell
}

__global__ void ious_sum_kernel(const float* __restrict__ hits, int B, float* __restrict__ out)
{
    const int t = threadIdx.x;
    if (t >= 8) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += hits[(size_t)b * 8 + t];
    out[t] = s;
}

// Closing pass of the epoch meter: one wave, thread per slot of acc [4 + npairs].  Each slot's batch sum is formed in fp64 over
// the samples in order, then added to the accumulator once (include/smin_hip.h gives the layout and the order).
__global__ __launch_bounds__(64)
void meter_close_kernel(const float* __restrict__ hits /* [B][npairs] */, const float* __restrict__ top1 /* [B] */, int B, int npairs,
                        const float* __restrict__ loss /* [1] or null */, double* __restrict__ acc)
{
#pragma clang fp contract(off)
    for (int slot = threadIdx.x; slot < 4 + npairs; slot += 64) {
        double s = 0.0;
        if (slot == 0) {
            s = (double)B;
        } else if (slot == 1 || slot == 2) {
            if (!loss) continue;
            s = slot == 1 ? (double)loss[0] * (double)B : (double)B;
        } else if (slot == 3) {
            for (int b = 0; b < B; ++b) s += (double)top1[b];
        } else {
            for (int b = 0; b < B; ++b) s += (double)hits[(size_t)b * npairs + (slot - 4)];
        }
        acc[slot] += s;
    }
}

// ---- span metric (smin_span_ious / smin_span_meter_update, include/smin_hip.h): R@n, IoU=m and the top-1 IoU of continuous spans
// (SMIN.localize_windows' merged output) against one ground-truth span per pair.  One lane per pair (k <= 64 slots), workgroups
// of one wave; the meter's per-pair stage keeps the lane's IoUs in an LDS column and the batch sums go through meter_close_kernel.

// IoU of slot (st, en) with (gs, ge): fp32, each operation rounded once; NaN operands leave through fminf / fmaxf and the uni > 0 test
__device__ __forceinline__ float span_iou(float st, float en, float gs, float ge)
{
    const float inter = fmaxf(0.f, fminf(en, ge) - fmaxf(st, gs));
    const float uni = fmaxf(en, ge) - fminf(st, gs);
    return uni > 0.f ? inter / uni : 0.f;
}

__global__ __launch_bounds__(64)
void span_ious_kernel(const float* __restrict__ span, const int* __restrict__ count, const float* __restrict__ gt, int B, int k,
                      float* __restrict__ iou /* [B][k] */)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float gs = gt[2 * (size_t)b], ge = gt[2 * (size_t)b + 1];
    const int cnt = min(max(count[b], 0), k);
    for (int s = 0; s < k; ++s) {
        const size_t o = (size_t)b * k + s;
        iou[o] = s < cnt ? span_iou(span[2 * o], span[2 * o + 1], gs, ge) : 0.f;       // an empty slot's NaN span is never read
    }
}

struct SpanRule { int n[64]; float m[16]; int nn, nm; };

__global__ __launch_bounds__(64)
void span_hits_kernel(const float* __restrict__ span, const int* __restrict__ count, const float* __restrict__ gt, int B, int k, SpanRule pr,
                      float* __restrict__ hits /* [B][nn * nm] */, float* __restrict__ top1 /* [B] */)
{
    __shared__ float col[64][64];                                // col[s][lane]: the lane's IoU of slot s (a column per lane: no bank conflict)
    const int t = threadIdx.x, b = blockIdx.x * 64 + t;
    if (b >= B) return;                                          // no barrier below: a lane reads its own column only
    const float gs = gt[2 * (size_t)b], ge = gt[2 * (size_t)b + 1];
    const int cnt = min(max(count[b], 0), k);
    for (int s = 0; s < cnt; ++s) {
        const size_t o = (size_t)b * k + s;
        col[s][t] = span_iou(span[2 * o], span[2 * o + 1], gs, ge);
    }
    top1[b] = cnt > 0 ? col[0][t] : 0.f;
    const int npairs = pr.nn * pr.nm;
    for (int a = 0; a < pr.nn; ++a) {
        const int e = min(pr.n[a], cnt);                         // slots past count[b] are empty: never a hit
        for (int c = 0; c < pr.nm; ++c) {
            bool hit = false;
            for (int s = 0; s < e; ++s) hit = hit || col[s][t] > pr.m[c];
            hits[(size_t)b * npairs + a * pr.nm + c] = hit ? 1.f : 0.f;
        }
    }
}

// ---- corpus metric (smin_corpus_meter_update, include/smin_hip.h): VCMR R@n, IoU=m, VR R@n and the top-1 IoU of SMIN.search-style
// ranked lists over a corpus against one ground-truth (video, span) per query.  The per-query stage of span_hits_kernel with the
// entry's video in the test: an entry of another video has IoU 0.
__global__ __launch_bounds__(64)
void corpus_hits_kernel(const long long* __restrict__ video, const float* __restrict__ span, const int* __restrict__ count,
                        const long long* __restrict__ gt_video, const float* __restrict__ gt, int Q, int k, SpanRule pr,
                        float* __restrict__ hits /* [Q][nn * nm + nn] */, float* __restrict__ top1 /* [Q] */)
{
    __shared__ float col[64][64];                                // col[r][lane]: the lane's IoU of entry r
    const int t = threadIdx.x, b = blockIdx.x * 64 + t;
    if (b >= Q) return;                                          // no barrier below: a lane reads its own column only
    const float gs = gt[2 * (size_t)b], ge = gt[2 * (size_t)b + 1];
    const long long gv = gt_video[b];
    const long long* vb = video + (size_t)b * k;
    const int cnt = min(max(count[b], 0), k);
    int first = -1;                                              // the first entry of the ground-truth video
    for (int r = 0; r < cnt; ++r) {
        const size_t o = (size_t)b * k + r;
        const bool same = vb[r] == gv;
        col[r][t] = same ? span_iou(span[2 * o], span[2 * o + 1], gs, ge) : 0.f;
        if (same && first < 0) first = r;
    }
    top1[b] = cnt > 0 ? col[0][t] : 0.f;
    const int npairs = pr.nn * pr.nm + pr.nn;
    float* hb = hits + (size_t)b * npairs;
    for (int a = 0; a < pr.nn; ++a) {
        const int e = min(pr.n[a], cnt);
        for (int c = 0; c < pr.nm; ++c) {
            bool hit = false;
            for (int r = 0; r < e; ++r) hit = hit || col[r][t] > pr.m[c];
            hb[a * pr.nm + c] = hit ? 1.f : 0.f;
        }
    }
    int distinct = 0;                                            // distinct videos ranked ahead of the ground-truth video
    for (int r = 0; r < first; ++r) {
        bool seen = false;
        for (int u = 0; u < r; ++u) seen = seen || vb[u] == vb[r];
        distinct += seen ? 0 : 1;
    }
    for (int a = 0; a < pr.nn; ++a) hb[pr.nn * pr.nm + a] = (first >= 0 && distinct < pr.n[a]) ? 1.f : 0.f;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// rule 0 is the reference's metric as this file computes it: n = {1, 5}, m = {0.1, 0.3, 0.5, 0.7}, topk(5) over all L*L cells
static bool rule0_shape_ok(int B, int L, int k, int nn, int nm)
{
    return B >= 1 && L >= 1 && (size_t)L * L >= 5 && (size_t)L * L < 0x7fffffff && k == 5 && nn == 2 && nm == 4;
}

}  // namespace smin

using namespace smin;

extern "C" int smin_compute_ious(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                 int B, int L, float* counts /* [8]: R@1 x {0.1,0.3,0.5,0.7}, R@5 x {...} */, float* ws /* [B][8] */)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(B >= 1 && L >= 1 && (size_t)L * L >= 5 && (size_t)L * L < 0x7fffffff);
    hipLaunchKernelGGL(ious_kernel, dim3(B), dim3(256), 0, st, pm, ps, pe, mm, sm, L, ws, (float*)nullptr);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(ious_sum_kernel, dim3(1), dim3(64), 0, st, ws, B, counts);
    SMIN_LAUNCH_CHECK();
    return 0;
}

// the meter's rule 1 under a selection rule (hard or soft): the per-sample stage of moments.hip with the top-1 IoU [B] behind its
// scratch, then the closing wave
static size_t meter_stage_ws_bytes(int method, int B, int L, int k, int nn, int nm)
{
    const size_t stage = rule_hits_stage_bytes(method, B, L, k, nn, nm);
    return stage ? stage + align256((size_t)B * sizeof(float)) : 0;
}

static int meter_stage_update(hipStream_t st, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm, int B, int L, int k,
                              const NmsRule& rule, const int* n_list, int nn, const float* m_list, int nm, const float* loss, double* acc, void* ws)
{
    float* hits = nullptr;
    float* top1 = (float*)((char*)ws + rule_hits_stage_bytes(rule.method, B, L, k, nn, nm));
    const int rc = rule_hits_stage(st, pm, ps, pe, mm, sm, B, L, k, rule, n_list, nn, m_list, nm, ws, &hits, top1);
    if (rc) return rc;
    hipLaunchKernelGGL(meter_close_kernel, dim3(1), dim3(64), 0, st, hits, top1, B, nn * nm, loss, acc);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_epoch_meter_ws_bytes(int B, int L, int rule, int k, int nn, int nm)
{
    if (rule == 0) return rule0_shape_ok(B, L, k, nn, nm) ? align256((size_t)B * 8 * sizeof(float)) + align256((size_t)B * sizeof(float)) : 0;
    return rule == 1 ? meter_stage_ws_bytes(0, B, L, k, nn, nm) : 0;
}

extern "C" int smin_epoch_meter_update(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                       int B, int L, int rule, int k, float nms_thresh, const int* n_list, int nn, const float* m_list, int nm,
                                       const float* loss, double* acc, void* ws, size_t ws_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(rule == 0 || rule == 1);
    SMIN_REQUIRE(n_list != nullptr && m_list != nullptr && acc != nullptr && ws != nullptr);
    const size_t need = smin_epoch_meter_ws_bytes(B, L, rule, k, nn, nm);
    SMIN_REQUIRE(need != 0 && ws_bytes >= need);
    if (rule == 1) return meter_stage_update(st, pm, ps, pe, mm, sm, B, L, k, NmsRule{0, nms_thresh, 0.f, 0.f}, n_list, nn, m_list, nm, loss, acc, ws);
    SMIN_REQUIRE(n_list[0] == 1 && n_list[1] == 5 && m_list[0] == 0.1f && m_list[1] == 0.3f && m_list[2] == 0.5f && m_list[3] == 0.7f);
    float* hits = (float*)ws;
    float* top1 = (float*)((char*)ws + align256((size_t)B * 8 * sizeof(float)));
    hipLaunchKernelGGL(ious_kernel, dim3(B), dim3(256), 0, st, pm, ps, pe, mm, sm, L, hits, top1);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(meter_close_kernel, dim3(1), dim3(64), 0, st, hits, top1, B, nn * nm, loss, acc);
    SMIN_LAUNCH_CHECK();
    return 0;
}

// the meter's rule 1 with a Soft-NMS selection (soft_nms.hip) in place of the greedy hard NMS
extern "C" size_t smin_epoch_meter_soft_ws_bytes(int B, int L, int k, int nn, int nm)
{
    return meter_stage_ws_bytes(SMIN_NMS_LINEAR, B, L, k, nn, nm);      // both soft rules carve the same scratch
}

extern "C" int smin_epoch_meter_update_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                            int B, int L, int k, int method, float nms_thresh, float sigma, const int* n_list, int nn,
                                            const float* m_list, int nm, const float* loss, double* acc, void* ws, size_t ws_bytes)
{
    const NmsRule rule{method, nms_thresh, sigma, -__builtin_inff()};
    SMIN_REQUIRE(soft_rule_ok(rule));
    SMIN_REQUIRE(pm != nullptr && ps != nullptr && pe != nullptr && mm != nullptr && sm != nullptr);
    SMIN_REQUIRE(n_list != nullptr && m_list != nullptr && acc != nullptr && ws != nullptr);
    const size_t need = smin_epoch_meter_soft_ws_bytes(B, L, k, nn, nm);
    SMIN_REQUIRE(need != 0 && ws_bytes >= need);
    return meter_stage_update((hipStream_t)stream, pm, ps, pe, mm, sm, B, L, k, rule, n_list, nn, m_list, nm, loss, acc, ws);
}

extern "C" int smin_span_ious(void* stream, const float* span, const int32_t* count, const float* gt, int B, int k, float* iou)
{
    SMIN_REQUIRE(B >= 0 && k >= 1 && k <= 64);
    if (B == 0) return 0;
    SMIN_REQUIRE(span != nullptr && count != nullptr && gt != nullptr && iou != nullptr);
    hipLaunchKernelGGL(span_ious_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, span, count, gt, B, k, iou);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_span_meter_ws_bytes(int B, int nn, int nm)
{
    if (B < 1 || nn < 1 || nn > 64 || nm < 1 || nm > 16) return 0;
    return align256((size_t)B * nn * nm * sizeof(float)) + align256((size_t)B * sizeof(float));
}

extern "C" int smin_span_meter_update(void* stream, const float* span, const int32_t* count, const float* gt, int B, int k,
                                      const int* n_list, int nn, const float* m_list, int nm, double* acc, void* ws, size_t ws_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(B >= 0 && k >= 1 && k <= 64 && nn >= 1 && nn <= 64 && nm >= 1 && nm <= 16 && n_list != nullptr && m_list != nullptr);
    SpanRule pr{};
    pr.nn = nn; pr.nm = nm;
    for (int a = 0; a < nn; ++a) { SMIN_REQUIRE(n_list[a] >= 1 && n_list[a] <= k); pr.n[a] = n_list[a]; }
    for (int c = 0; c < nm; ++c) pr.m[c] = m_list[c];
    if (B == 0) return 0;
    SMIN_REQUIRE(span != nullptr && count != nullptr && gt != nullptr && acc != nullptr && ws != nullptr);
    SMIN_REQUIRE(ws_bytes >= smin_span_meter_ws_bytes(B, nn, nm));
    float* hits = (float*)ws;
    float* top1 = (float*)((char*)ws + align256((size_t)B * nn * nm * sizeof(float)));
    hipLaunchKernelGGL(span_hits_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, span, count, gt, B, k, pr, hits, top1);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(meter_close_kernel, dim3(1), dim3(64), 0, st, hits, top1, B, nn * nm, (const float*)nullptr, acc);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_corpus_meter_ws_bytes(int Q, int nn, int nm)
{
    if (Q < 1 || nn < 1 || nn > 64 || nm < 1 || nm > 16) return 0;
    return align256((size_t)Q * (nn * nm + nn) * sizeof(float)) + align256((size_t)Q * sizeof(float));
}

extern "C" int smin_corpus_meter_update(void* stream, const int64_t* video, const float* span, const int32_t* count, const int64_t* gt_video,
                                        const float* gt, int Q, int k, const int* n_list, int nn, const float* m_list, int nm, double* acc,
                                        void* ws, size_t ws_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(Q >= 0 && k >= 1 && k <= 64 && nn >= 1 && nn <= 64 && nm >= 1 && nm <= 16 && n_list != nullptr && m_list != nullptr);
    SpanRule pr{};
    pr.nn = nn; pr.nm = nm;
    for (int a = 0; a < nn; ++a) { SMIN_REQUIRE(n_list[a] >= 1 && n_list[a] <= k); pr.n[a] = n_list[a]; }
    for (int c = 0; c < nm; ++c) pr.m[c] = m_list[c];
    if (Q == 0) return 0;
    SMIN_REQUIRE(video != nullptr && span != nullptr && count != nullptr && gt_video != nullptr && gt != nullptr && acc != nullptr && ws != nullptr);
    SMIN_REQUIRE(ws_bytes >= smin_corpus_meter_ws_bytes(Q, nn, nm));
    const int npairs = nn * nm + nn;
    float* hits = (float*)ws;
    float* top1 = (float*)((char*)ws + align256((size_t)Q * npairs * sizeof(float)));
    hipLaunchKernelGGL(corpus_hits_kernel, dim3(cdiv(Q, 64)), dim3(64), 0, st, (const long long*)video, span, count, (const long long*)gt_video, gt, Q, k,
                       pr, hits, top1);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(meter_close_kernel, dim3(1), dim3(64), 0, st, hits, top1, Q, npairs, (const float*)nullptr, acc);
    SMIN_LAUNCH_CHECK();
    return 0;
}
