// The window plan of a pruned window search: from each query's surviving videos (smin_prefilter_select's sel_video)
// and the bank's video_ptr to the (query, window) list and its group pointers, where search_windows builds them on the host when the
// host chooses the pairs.
//   smin_window_expand  three launches, no workgroup waits on another:
//     1. one workgroup per query scans the window counts of its Ms groups in tiles of 256 (rank_order.h's block_scan_count): group_ptr
//        [q Ms + j] = the windows of the query's groups in front of j, for j >= 1; the query's total goes to the slot of j = 0, whose
//        own prefix is 0 by definition;
//     2. one workgroup scans the Q totals in tiles: the slot of j = 0 becomes the query's first slot, clamped to cap; group_ptr[Q Ms] and
//        total;
//     3. one workgroup per group adds its query's first slot to its prefix (clamped to cap: where the query's first slot was clamped
//        every sum is >= cap, so the clamped sum is the clamped truth) and writes its slots; cap / 256 more workgroups write the
//        padding.  A workgroup reads its query's j = 0 slot, which no workgroup of this launch writes, and its own slot.
// Integers only, no atomics, plain stores, every output element written, nothing written at or past cap.
#include "common.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int WT = 256;                      // threads of a workgroup
static_assert(WT == 256, "rank_order.h's block helpers are written for four waves");
typedef long long i64;

// the windows of a surviving video as [lo, hi) inside [0, W]: an entry outside [0, V) owns none, and a video_ptr that is no window
// plan (descending, outside the bank) is clamped, so every window written is a window of the bank
__device__ __forceinline__ void group_windows(int v, const int64_t* __restrict__ video_ptr, int V, i64 W, i64& lo, i64& hi)
{
    lo = hi = 0;
    if (v < 0 || v >= V) return;
    lo = min(max((i64)video_ptr[v], (i64)0), W);
    hi = min(max((i64)video_ptr[v + 1], lo), W);
}

__global__ __launch_bounds__(WT)
void window_expand_scan_kernel(const int* __restrict__ sel_video, const int64_t* __restrict__ video_ptr, int Ms, int V, i64 W,
                               int64_t* __restrict__ group_ptr)
{
    __shared__ i64 red[4];
    const int q = blockIdx.x, t = threadIdx.x;
    const size_t g0 = (size_t)q * Ms;
    i64 before = 0, total;
    for (int j0 = 0; j0 < Ms; j0 += WT) {
        const int j = j0 + t;
        i64 lo = 0, hi = 0;
        if (j < Ms) group_windows(sel_video[g0 + j], video_ptr, V, W, lo, hi);
        const i64 at = before + block_scan_count(hi - lo, red, total);
        before += total;
        if (j < Ms && j > 0) group_ptr[g0 + j] = at;
    }
    if (t == 0) group_ptr[g0] = before;
}

__global__ __launch_bounds__(WT)
void window_expand_offsets_kernel(int Q, int Ms, i64 cap, int64_t* __restrict__ group_ptr, int64_t* __restrict__ total_out)
{
    __shared__ i64 red[4];
    const int t = threadIdx.x;
    i64 before = 0, total;
    for (int q0 = 0; q0 < Q; q0 += WT) {
        const int q = q0 + t;
        const i64 n = q < Q ? (i64)group_ptr[(size_t)q * Ms] : 0;
        const i64 at = before + block_scan_count(n, red, total);
        before += total;
        if (q < Q) group_ptr[(size_t)q * Ms] = min(at, cap);
    }
    if (t == 0) {
        group_ptr[(size_t)Q * Ms] = min(before, cap);
        total_out[0] = before;
    }
}

__global__ __launch_bounds__(WT)
void window_expand_fill_kernel(const int* __restrict__ sel_video, const int64_t* __restrict__ video_ptr, int G, int Ms, int V, i64 W, i64 cap,
                               int64_t* __restrict__ group_ptr, int* __restrict__ win_index, int* __restrict__ win_query)
{
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= G) {                                  // the padding: a real window and a real query that no group owns
        const i64 s = (i64)(blockIdx.x - G) * WT + t;
        if (s >= (i64)group_ptr[G] && s < cap) {
            win_index[s] = 0;
            win_query[s] = 0;
        }
        return;
    }
    const int g = blockIdx.x, q = g / Ms, j = g - q * Ms;
    i64 begin = group_ptr[(size_t)q * Ms];
    if (j > 0) {
        begin = min(begin + (i64)group_ptr[g], cap);
        __syncthreads();                                         // (every thread has read the prefix this slot held)
        if (t == 0) group_ptr[g] = begin;
    }
    i64 lo, hi;
    group_windows(sel_video[g], video_ptr, V, W, lo, hi);
    const i64 n = min(hi - lo, cap - begin);
    for (i64 i = t; i < n; i += WT) {
        win_index[begin + i] = (int)(lo + i);
        win_query[begin + i] = q;
    }
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" int smin_window_expand(void* stream, const int32_t* sel_video, const int64_t* video_ptr, int Q, int Ms, int V, int64_t W, int64_t cap,
                                  int64_t* group_ptr, int32_t* win_index, int32_t* win_query, int64_t* total)
{
    SMIN_REQUIRE(Q >= 0 && Ms >= 0 && V >= 0 && W >= 0 && W < (1ll << 31) && cap >= 0 && cap < (1ll << 31));
    SMIN_REQUIRE((long long)Q * Ms <= 0x7f000000ll);             // (the fill's grid: a workgroup per group and cap / 256 more)
    if (Q == 0 || Ms == 0) return 0;
    SMIN_REQUIRE(sel_video && video_ptr && group_ptr && total && (cap == 0 || (win_index && win_query)));
    const hipStream_t st = (hipStream_t)stream;
    const int G = Q * Ms;
    hipLaunchKernelGGL(window_expand_scan_kernel, dim3(Q), dim3(WT), 0, st, sel_video, video_ptr, Ms, V, (i64)W, group_ptr);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(window_expand_offsets_kernel, dim3(1), dim3(WT), 0, st, Q, Ms, (i64)cap, group_ptr, total);
    SMIN_LAUNCH_CHECK();
    const unsigned pad_groups = (unsigned)((cap + WT - 1) / WT);
    hipLaunchKernelGGL(window_expand_fill_kernel, dim3((unsigned)G + pad_groups), dim3(WT), 0, st, sel_video, video_ptr, G, Ms, V, (i64)W, (i64)cap,
                       group_ptr, win_index, win_query);
    SMIN_LAUNCH_CHECK();
    return 0;
}
