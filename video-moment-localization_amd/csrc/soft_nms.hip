// Soft-NMS moment retrieval: top-k where every pick decays the score of the candidates it overlaps, and the rest is ranked again.
//
// Candidates, score formula, IoU, order word (ties -> lower flat index, -0 counts as +0), empty slots and the limits on B, L and k are
// those of moments.hip's header (moment_cells.h holds the one copy of each).  Per sample, with cur(c) = s0(c) initially:
//   pick    the remaining candidate with the highest cur, by the order word of cur, then the lower flat index;
//   stop    after k picks, when no candidate is left, or when the best cur < min_score (fp32; min_score = -inf never stops early);
//   record  idx, score = cur at pick time, raw_score = s0 of the picked cell (a zero of either sign is written as +0);
//   decay   for every remaining candidate: iou with the pick (one correctly rounded fp32 division), then cur = cur * w as one fp32
//           multiplication, never contracted into an fma:
//             SMIN_NMS_LINEAR    w = iou > nms_thresh ? 1.0f - iou : 1.0f
//             SMIN_NMS_GAUSSIAN  w = expf(-(iou * iou) / sigma) for every candidate; sigma > 0, +inf allowed (w = 1)
//   The decays are applied in pick order, cur = ((s0 * w1) * w2) ..., one candidate's chain in one thread: the result does not depend
//   on how the cells are split over threads, bands or launches.  The linear rule uses correctly rounded fp32 operations only and is
//   reproducible bit for bit anywhere; the gaussian rule is as exact as the device library's expf.
//   Signed scores follow the same formulas.  NaN and +-inf at VALID cells are out of scope for the soft rules (a decay of 0 * inf
//   is NaN, and a cur whose bits are 0xffffffff is taken for a removed cell); NaN and inf at MASKED cells are never read into the order.
//
// cur is one 32-bit word per cell: the fp32 bits, or GONE for a masked or already picked cell.
//
// Dispatch (no workgroup waits on another; stage order comes from kernel boundaries only; no float atomics, no host read):
//   L * L <= LDS_CELLS  one launch, one workgroup per sample: cur in LDS, k rounds of block argmax + decay of the workgroup's cells.
//   larger maps         k + 1 launches over the band grid (P, B), cur [B][L*L] and two ping-pong band-best buffers [B][P] in the
//                       workspace.  Launch 0 forms cur and each band's best key.  Launch r = 1 .. k: every band workgroup reduces
//                       the P band-bests of launch r - 1 to pick r - 1 (band 0 records it), decays its own band and writes its new
//                       best into the other buffer.  A stopped sample writes 0 keys, so it stays stopped.  Launch k only records.
//   span form           one workgroup per pair, k rounds; every round recomputes each candidate's cur from the kept spans in pick order
//                       (like merge_windows_kernel), so it needs no workspace.
#include "common.h"
#include "moment_cells.h"
#include "rank_order.h"
#include "smin_hip.h"

#include <algorithm>
#include <cmath>

namespace smin {
namespace {

constexpr int MT = MOMENT_THREADS;
static_assert(MT == 256, "rank_order.h's block helpers are written for four waves");
constexpr int MAX_K = MOMENT_MAX_K;
constexpr int LDS_CELLS = 12288;        // a sample's cur fits in LDS up to here (48 KiB): L <= 110
constexpr int BAND_CELLS = 4096;        // banded path: cells per band at least ...
constexpr int MAX_BANDS = 32;           // ... and at most this many bands per sample
constexpr uint32_t GONE = 0xffffffffu;  // cur word of a masked or picked cell

__device__ __forceinline__ float decayed(float cur, float iou, const NmsRule& r)
{
#pragma clang fp contract(off)
    float w;
    if (r.method == SMIN_NMS_LINEAR) w = iou > r.thr ? 1.0f - iou : 1.0f;
    else w = expf(-(iou * iou) / r.sigma);
    return cur * w;
}

__device__ __forceinline__ float plus_zero(float v) { return v == 0.f ? 0.f : v; }

// cur word of cell c at the start: its score (-0 -> +0), GONE if it is masked
__device__ __forceinline__ uint32_t first_word(const Map& m, int c, int i, int j)
{
    return m.mm[c] ? __float_as_uint(plus_zero(cell_score(m, c, i, j))) : GONE;
}

__device__ __forceinline__ u64 word_key(uint32_t w, int c) { return w == GONE ? 0ull : make_key(score_ord(__uint_as_float(w)), c); }

// one round over the cells [lo, hi) of a sample: the pick leaves, every other remaining cell is decayed; returns the thread's best key
template <typename W>
__device__ __forceinline__ u64 decay_cells(const Map& m, W* cur, int lo, int hi, int pick, const NmsRule& rule)
{
    const int pi = pick / m.L, pj = pick - pi * m.L;
    u64 best = 0;
    for_cells(m, lo, hi, [&](int c, int i, int j) {
        const uint32_t w = cur[c];
        if (w == GONE) return;
        if (c == pick) { cur[c] = GONE; return; }
        const uint32_t d = __float_as_uint(decayed(__uint_as_float(w), cell_iou(i, j, pi, pj), rule));
        cur[c] = d;
        const u64 key = word_key(d, c);
        best = key > best ? key : best;
    });
    return best;
}

struct Out { long long* idx; float* score; float* raw; int* count; };

__device__ __forceinline__ void write_pick(const Out& o, const Map& m, size_t slot, int c, float v)
{
    const int i = c / m.L, j = c - i * m.L;
    o.idx[2 * slot] = i; o.idx[2 * slot + 1] = j;
    o.score[slot] = plus_zero(v);
    o.raw[slot] = plus_zero(cell_score(m, c, i, j));
}
__device__ __forceinline__ void write_empty(const Out& o, size_t slot)
{
    o.idx[2 * slot] = -1; o.idx[2 * slot + 1] = -1; o.score[slot] = 0.f; o.raw[slot] = 0.f;
}

__global__ __launch_bounds__(MT)
void soft_top_lds_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                         const uint8_t* __restrict__ mm, int L, int k, NmsRule rule, Out out)
{
    __shared__ uint32_t cur[LDS_CELLS];
    __shared__ u64 red[MT / 64];
    const int b = blockIdx.x, t = threadIdx.x, n = L * L;
    const size_t o = (size_t)b * n;
    const Map m{pm + o, ps + (size_t)b * L, pe + (size_t)b * L, mm + o, L, n};
    u64 best = 0;
    for_cells(m, 0, n, [&](int c, int i, int j) {                // a thread owns the cells c = t (mod MT) in every round
        const uint32_t w = first_word(m, c, i, j);
        cur[c] = w;
        const u64 key = word_key(w, c);
        best = key > best ? key : best;
    });
    int nk = 0;
    while (nk < k) {
        const u64 top = block_max(best, red);
        if (top == 0) break;                                     // no candidate left
        const int c = key_cell(top);
        const float v = __uint_as_float(cur[c]);
        if (v < rule.min_score) break;
        if (t == 0) write_pick(out, m, (size_t)b * k + nk, c, v);
        ++nk;
        if (nk == k) break;
        __syncthreads();                                         // every thread has read cur[c] before its owner removes it
        best = decay_cells(m, cur, 0, n, c, rule);
    }
    for (int r = nk + t; r < k; r += MT) write_empty(out, (size_t)b * k + r);
    if (t == 0) out.count[b] = nk;
}

// ---- banded path
__global__ __launch_bounds__(MT)
void soft_band_init_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                           const uint8_t* __restrict__ mm, int L, int P, uint32_t* __restrict__ cur /* [B][n] */,
                           u64* __restrict__ best_out /* [B][P] */, int* __restrict__ count)
{
    __shared__ u64 red[MT / 64];
    const int p = blockIdx.x, b = blockIdx.y, n = L * L;
    const size_t o = (size_t)b * n;
    const Map m{pm + o, ps + (size_t)b * L, pe + (size_t)b * L, mm + o, L, n};
    const int band = (n + P - 1) / P, lo = min(p * band, n), hi = min(lo + band, n);
    uint32_t* cb = cur + o;
    u64 best = 0;
    for_cells(m, lo, hi, [&](int c, int i, int j) {
        const uint32_t w = first_word(m, c, i, j);
        cb[c] = w;
        const u64 key = word_key(w, c);
        best = key > best ? key : best;
    });
    best = block_max(best, red);
    if (threadIdx.x == 0) {
        best_out[(size_t)b * P + p] = best;
        if (p == 0) count[b] = 0;
    }
}

// launch r (1 .. k): pick r - 1 from the band-bests of launch r - 1, then this band's decay and its new best
__global__ __launch_bounds__(MT)
void soft_band_round_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                            const uint8_t* __restrict__ mm, int L, int P, int k, int r, NmsRule rule, uint32_t* __restrict__ cur,
                            const u64* __restrict__ best_in, u64* __restrict__ best_out, Out out)
{
    __shared__ u64 red[MT / 64];
    const int p = blockIdx.x, b = blockIdx.y, t = threadIdx.x, n = L * L;
    const size_t o = (size_t)b * n;
    const Map m{pm + o, ps + (size_t)b * L, pe + (size_t)b * L, mm + o, L, n};
    u64 top = 0;
    for (int q = 0; q < P; ++q) { const u64 x = best_in[(size_t)b * P + q]; top = x > top ? x : top; }
    const float v = ord_score((uint32_t)(top >> 32));            // cur of the pick (a zero as +0)
    const bool stopped = top == 0 || v < rule.min_score;
    const size_t slot = (size_t)b * k + (r - 1);
    if (p == 0 && t == 0) {
        if (stopped) write_empty(out, slot);
        else { write_pick(out, m, slot, key_cell(top), v); out.count[b] = r; }
    }
    if (r == k) return;                                          // the last launch only records
    u64 best = 0;
    if (!stopped) {                                              // (uniform over the workgroup)
        const int band = (n + P - 1) / P, lo = min(p * band, n), hi = min(lo + band, n);
        best = decay_cells(m, cur + o, lo, hi, key_cell(top), rule);
    }
    best = block_max(best, red);
    if (t == 0) best_out[(size_t)b * P + p] = best;              // 0 once stopped: the sample stays stopped
}

int band_count(int L)
{
    const long long n = (long long)L * L;
    return (int)std::min<long long>(MAX_BANDS, (n + BAND_CELLS - 1) / BAND_CELLS);
}

struct WsLayout { int P; size_t cur, best0, best1, total; };

// The LDS-resident path carves nothing; it reports one 256-byte unit so that 0 keeps meaning "arguments rejected".
WsLayout ws_layout(int B, int L)
{
    WsLayout w{};
    const size_t n = (size_t)L * L;
    if (n <= (size_t)LDS_CELLS) { w.P = 0; w.total = 256; return w; }
    w.P = band_count(L);
    w.cur = 0;
    w.best0 = moment_align256((size_t)B * n * sizeof(uint32_t));
    w.best1 = w.best0 + moment_align256((size_t)B * w.P * sizeof(u64));
    w.total = w.best1 + moment_align256((size_t)B * w.P * sizeof(u64));
    return w;
}

// ---- span form: the candidates, spans and span IoU of merge_windows_kernel (moment_cells.h), the soft rule in place of the threshold
__global__ __launch_bounds__(MT)
void soft_merge_windows_kernel(MergeIn in, const long long* __restrict__ pair_ptr, int k, NmsRule rule, MergeOut out)
{
    __shared__ float kst[MAX_K], ken[MAX_K];
    __shared__ int kq[MAX_K];
    __shared__ float pick_cur;
    __shared__ u64 red[MT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const MergePair pr = merge_pair(in, pair_ptr, b);
    int nk = 0;
    for (; nk < k; ++nk) {
        u64 best = 0;
        float best_cur = 0.f;
        for (int q = t; q < pr.nslot; q += MT) {
            const MergeCand x = merge_cand(in, pr.g0, q);
            if (x.slot >= in.count[x.g]) continue;
            float st, en;
            cand_span(in, x, st, en);
            float cur = in.score[x.c];
            bool taken = false;
            for (int r = 0; r < nk; ++r) {                       // the decays in pick order
                taken = taken || kq[r] == q;
                cur = decayed(cur, span_iou(st, en, kst[r], ken[r]), rule);
            }
            if (taken) continue;
            const u64 key = make_key(score_ord(cur), q);
            if (key > best) { best = key; best_cur = cur; }
        }
        const u64 top = block_max(best, red);
        if (top == 0) break;                                     // every candidate is taken
        if (best == top) pick_cur = best_cur;                    // keys are distinct per candidate: one thread
        __syncthreads();
        const float v = pick_cur;
        if (v < rule.min_score) break;
        if (t == 0) {
            kq[nk] = key_cell(top);
            merge_record(in, out, pr.g0, kq[nk], (size_t)b * k + nk, v, kst[nk], ken[nk]);
        }
        __syncthreads();
    }
    merge_finish(out, b, k, nk);
}

}  // namespace

bool soft_rule_ok(const NmsRule& rule)
{
    if (rule.method == SMIN_NMS_LINEAR) return true;
    return rule.method == SMIN_NMS_GAUSSIAN && rule.sigma > 0.f;  // (false for a NaN sigma)
}

size_t soft_top_ws_total(int B, int L) { return ws_layout(B, L).total; }

int soft_top_launch(hipStream_t st, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k, const NmsRule& rule,
                    long long* idx, float* score, float* raw_score, int* count, char* ws)
{
    const WsLayout w = ws_layout(B, L);
    const Out out{idx, score, raw_score, count};
    if (w.P == 0) {
        hipLaunchKernelGGL(soft_top_lds_kernel, dim3(B), dim3(MT), 0, st, pm, ps, pe, mm, L, k, rule, out);
        SMIN_LAUNCH_CHECK();
        return 0;
    }
    uint32_t* cur = (uint32_t*)(ws + w.cur);
    u64* best[2] = {(u64*)(ws + w.best0), (u64*)(ws + w.best1)};
    hipLaunchKernelGGL(soft_band_init_kernel, dim3(w.P, B), dim3(MT), 0, st, pm, ps, pe, mm, L, w.P, cur, best[0], count);
    SMIN_LAUNCH_CHECK();
    for (int r = 1; r <= k; ++r) {
        hipLaunchKernelGGL(soft_band_round_kernel, dim3(w.P, B), dim3(MT), 0, st, pm, ps, pe, mm, L, w.P, k, r, rule, cur,
                           (const u64*)best[(r - 1) & 1], best[r & 1], out);
        SMIN_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace smin

using namespace smin;

extern "C" size_t smin_top_moments_soft_ws_bytes(int B, int L, int k)
{
    if (!moment_args_ok(B, L, k)) return 0;
    return ws_layout(B, L).total;
}

extern "C" int smin_top_moments_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k,
                                     int method, float nms_thresh, float sigma, float min_score, long long* idx, float* score,
                                     float* raw_score, int* count, void* ws, size_t ws_bytes)
{
    const NmsRule rule{method, nms_thresh, sigma, min_score};
    SMIN_REQUIRE(soft_rule_ok(rule));
    SMIN_REQUIRE(moment_args_ok(B, L, k));
    SMIN_REQUIRE(pm != nullptr && ps != nullptr && pe != nullptr && mm != nullptr);
    SMIN_REQUIRE(idx != nullptr && score != nullptr && raw_score != nullptr && count != nullptr);
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= ws_layout(B, L).total);
    return soft_top_launch((hipStream_t)stream, pm, ps, pe, mm, B, L, k, rule, idx, score, raw_score, count, (char*)ws);
}

extern "C" int smin_merge_window_moments_soft(void* stream, const int64_t* idx, const float* score, const int32_t* count, const int64_t* start,
                                              const int32_t* len, const int64_t* pair_ptr, int G, int B, int T, int L, int k_window, int k,
                                              int method, float nms_thresh, float sigma, float min_score, float* span, float* out_score,
                                              float* raw_score, int64_t* window, int64_t* cell, int32_t* out_count)
{
    const NmsRule rule{method, nms_thresh, sigma, min_score};
    SMIN_REQUIRE(soft_rule_ok(rule));
    const MergeIn in{(const long long*)idx, score, count, (const long long*)start, len, G, T, L, k_window};
    const MergeOut out{span, out_score, raw_score, (long long*)window, (long long*)cell, out_count};
    SMIN_REQUIRE(merge_args_ok(in, pair_ptr, B, k, out) && (B == 0 || raw_score != nullptr));
    if (B == 0) return 0;
    hipLaunchKernelGGL(soft_merge_windows_kernel, dim3(B), dim3(MT), 0, (hipStream_t)stream, in, (const long long*)pair_ptr, k, rule, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}
