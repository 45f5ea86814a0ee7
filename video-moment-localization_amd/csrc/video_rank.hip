// Video ranking by the pooled pair score: the retrieval side of the score pair_rank.hip trains.
//   smin_pair_pool        pools each (video, query) map into its pair score s_p -- pair_pool.h, the device code of smin_pair_rank_fwd's
//                         pool launch, so the bits are the loss's -- and keeps { m_p, the sum } and the valid-cell count beside it;
//   smin_group_pool       composes the pools of a (query, video) group's windows into the score of the group (window banks);
//   smin_video_rank       ranks, per query, its videos by that score: every pair's rank (by counting, no sort), the first n videos, each
//                         pair's weight exp(alpha * (s_p - s_max)) and the rank of the query's own video;
//   smin_moment_reweight  multiplies the pairs' moment lists by their weights and empties the lists of the videos behind max_videos;
//                         smin_corpus_topk / smin_corpus_span_topk then rank the lists as they are.
// No atomics, plain stores, every output element written, every sum in an order that depends on the arguments only.
#include <cmath>

#include "common.h"
#include "pair_pool.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int VT = 256;                      // threads of a workgroup
static_assert(VT == 256, "rank_order.h's block helpers are written for four waves");
constexpr int VR_TILE = 2048;                // order words of a segment staged in LDS at a time (16 KB)
constexpr int VR_OWN = 4;                    // pairs a thread ranks per pass over the segment: one LDS read serves them all
constexpr int VR_MAX_N = 64;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(VT)
void pair_pool_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe, const uint8_t* __restrict__ mm,
                      int L, float tau, float* __restrict__ score, float* __restrict__ pool, float* __restrict__ cells)
{
    __shared__ float red[4];
    const int p = blockIdx.x;
    const PairPool r = pair_pool_cells(pm, ps, pe, mm, p, L, tau, red);
    if (threadIdx.x == 0) {
        score[p] = r.score;
        pool[2 * (size_t)p] = r.m;
        pool[2 * (size_t)p + 1] = r.sum;
        cells[p] = r.cnt;
    }
}

// One thread per group, its windows in ascending order: the maximum over the windows with cells first, then the sum and the count.
__global__ __launch_bounds__(VT)
void group_pool_kernel(const float* __restrict__ pool, const float* __restrict__ cells, const int* __restrict__ group_ptr, int G2, int W, float tau,
                       float* __restrict__ score, float* __restrict__ out_cells)
{
    const int g = blockIdx.x * VT + threadIdx.x;
    if (g >= G2) return;
    const int w0 = clampi(group_ptr[g], 0, W), w1 = clampi(group_ptr[g + 1], w0, W);
    float M = -INFINITY, N = 0.f;
    for (int w = w0; w < w1; ++w)
        if (cells[w] > 0.f) { M = fmaxf(M, pool[2 * (size_t)w]); N += cells[w]; }
    float S = 0.f;
    for (int w = w0; w < w1; ++w)
        if (cells[w] > 0.f) S += pool[2 * (size_t)w + 1] * expf((pool[2 * (size_t)w] - M) / tau);
    score[g] = N > 0.f ? M + tau * logf(S / N) : 0.f;
    out_cells[g] = N;
}

// The order word of a candidate, larger = earlier: smin_corpus_topk's Key::hi (score, lower video); 0 for a pair that is no candidate.
__device__ __forceinline__ u64 rank_word(float score, float cells, int video)
{
    return cells > 0.f ? video_word(score, video) : 0ull;
}

// One workgroup per query over its segment [beg, end) of the pair lists.  Pass 1: the number of candidates and their best score.
// Pass 2, for the thread's own pairs e = beg + t, beg + t + 256, ... (VR_OWN at a time): the segment's order words go through LDS
// VR_TILE at a time and the pair counts the candidates ahead of it -- a larger word, or an equal word earlier in the list: a strict
// total order, so the candidates' ranks are a permutation of 0 .. ncand - 1 and each of the first n output slots has one writer.
// Slots ncand .. n - 1 are written empty.  Workgroup 0 also writes the pairs in front of the first segment and workgroup Q - 1 those
// behind the last as non-candidates: with an ascending pair_ptr every element of pair_rank and weight is written, by one workgroup.
// (A pair_ptr that is not ascending stays in bounds through the clamps, but its segments may overlap or leave gaps: smin_hip.h.)
__global__ __launch_bounds__(VT)
void video_rank_kernel(const float* __restrict__ pair_score, const float* __restrict__ pair_cells, const int* __restrict__ pair_video,
                       const int* __restrict__ pair_ptr, const int* __restrict__ gt_video, int P, int Q, int n, float alpha,
                       long long* __restrict__ out_video, float* __restrict__ out_score, int* __restrict__ out_count, int* __restrict__ pair_rank,
                       float* __restrict__ weight, int* __restrict__ gt_rank)
{
    __shared__ u64 tile[VR_TILE];
    __shared__ float redf[4];
    __shared__ int redi[4];
    const int q = blockIdx.x, t = threadIdx.x;
    const int beg = clampi(pair_ptr[q], 0, P), end = clampi(pair_ptr[q + 1], beg, P);
    if (q == 0) for (int e = t; e < beg; e += VT) { pair_rank[e] = -1; weight[e] = 0.f; }
    if (q == Q - 1) for (int e = end + t; e < P; e += VT) { pair_rank[e] = -1; weight[e] = 0.f; }
    int mine_n = 0;
    float smax = -INFINITY;
    for (int e = beg + t; e < end; e += VT)
        if (pair_cells[e] > 0.f) { ++mine_n; smax = fmaxf(smax, pair_score[e]); }
    const int ncand = block_sum(mine_n, redi);
    smax = rank_block_max(smax, redf);
    const int nk = min(ncand, n);
    const bool has_gt = gt_video != nullptr;
    const int gt = has_gt ? gt_video[q] : 0;
    int best_gt = 0x7fffffff;
    for (int own0 = beg; own0 < end; own0 += VT * VR_OWN) {      // (uniform trip count: the barriers below are reached by all)
        u64 mine[VR_OWN];
        float s[VR_OWN];
        int vid[VR_OWN], rank[VR_OWN];
#pragma unroll
        for (int r = 0; r < VR_OWN; ++r) {
            const int e = own0 + r * VT + t;
            const bool own = e < end;
            s[r] = own ? pair_score[e] : 0.f;
            vid[r] = own ? pair_video[e] : 0;
            mine[r] = own ? rank_word(s[r], pair_cells[e], vid[r]) : 0ull;
            rank[r] = 0;
        }
        for (int t0 = beg; t0 < end; t0 += VR_TILE) {
            const int tn = min(VR_TILE, end - t0);
            __syncthreads();                                     // (the previous tile's reads are done)
            for (int j = t; j < tn; j += VT) tile[j] = rank_word(pair_score[t0 + j], pair_cells[t0 + j], pair_video[t0 + j]);
            __syncthreads();
            for (int j = 0; j < tn; ++j) {                       // one LDS read (a broadcast) serves the thread's VR_OWN pairs
                const u64 w = tile[j];
#pragma unroll
                for (int r = 0; r < VR_OWN; ++r) rank[r] += (w > mine[r]) || (w == mine[r] && t0 + j < own0 + r * VT + t);
            }
        }
#pragma unroll
        for (int r = 0; r < VR_OWN; ++r) {
            const int e = own0 + r * VT + t;
            if (e >= end) continue;
            if (mine[r] == 0ull) { pair_rank[e] = -1; weight[e] = 0.f; continue; }   // (its count is not a rank: never read)
            pair_rank[e] = rank[r];
            weight[e] = alpha == 0.f ? 1.f : expf(alpha * (s[r] - smax));
            if (rank[r] < nk) {
                const size_t o = (size_t)q * n + rank[r];
                out_video[o] = vid[r];
                out_score[o] = s[r];
            }
            if (has_gt && vid[r] == gt) best_gt = min(best_gt, rank[r]);
        }
    }
    for (int r = nk + t; r < n; r += VT) {
        const size_t o = (size_t)q * n + r;
        out_video[o] = -1;
        out_score[o] = 0.f;
    }
    best_gt = block_min(best_gt, redi);
    if (t == 0) {
        out_count[q] = nk;
        gt_rank[q] = best_gt == 0x7fffffff ? -1 : best_gt;
    }
}

// One thread per slot of the P lists; the thread of slot 0 also writes the pair's count.
__global__ __launch_bounds__(VT)
void moment_reweight_kernel(const float* __restrict__ score, const int* __restrict__ count, const int* __restrict__ pair_rank, const float* __restrict__ weight,
                            size_t total, int k, int max_videos, float* __restrict__ out_score, int* __restrict__ out_count)
{
    const size_t idx = (size_t)blockIdx.x * VT + threadIdx.x;
    if (idx >= total) return;
    const size_t p = idx / k;
    out_score[idx] = score[idx] * weight[p];
    if (idx - p * k == 0) {
        const int r = pair_rank[p];
        out_count[p] = max_videos <= 0 || (r >= 0 && r < max_videos) ? count[p] : 0;
    }
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" int smin_pair_pool(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int P, int L, float tau,
                              float* score, float* pool, float* cells)
{
    SMIN_REQUIRE(P >= 1 && L >= 1 && L <= RANK_MAX_L);
    SMIN_REQUIRE(pm && ps && pe && mm && score && pool && cells);
    SMIN_REQUIRE(rank_temperature(tau));
    hipLaunchKernelGGL(pair_pool_kernel, dim3(P), dim3(VT), 0, (hipStream_t)stream, pm, ps, pe, mm, L, tau, score, pool, cells);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_group_pool(void* stream, const float* pool, const float* cells, const int32_t* group_ptr, int G2, int W, float tau,
                               float* score, float* out_cells)
{
    SMIN_REQUIRE(G2 >= 0 && W >= 0 && rank_temperature(tau));
    if (G2 == 0) return 0;
    SMIN_REQUIRE(group_ptr && score && out_cells && (W == 0 || (pool && cells)));
    hipLaunchKernelGGL(group_pool_kernel, dim3(cdiv(G2, VT)), dim3(VT), 0, (hipStream_t)stream, pool, cells, group_ptr, G2, W, tau, score, out_cells);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_video_rank(void* stream, const float* pair_score, const float* pair_cells, const int32_t* pair_video, const int32_t* pair_ptr,
                               const int32_t* gt_video, int P, int Q, int n, float alpha, int64_t* out_video, float* out_score, int32_t* out_count,
                               int32_t* pair_rank, float* weight, int32_t* gt_rank)
{
    SMIN_REQUIRE(P >= 0 && P <= 0x7fff0000 && Q >= 0 && n >= 1 && n <= VR_MAX_N && std::isfinite(alpha));   // (e + 256, t0 + VR_TILE stay int)
    if (Q == 0) return 0;
    SMIN_REQUIRE(pair_ptr && out_video && out_score && out_count && gt_rank);
    SMIN_REQUIRE(P == 0 || (pair_score && pair_cells && pair_video && pair_rank && weight));
    hipLaunchKernelGGL(video_rank_kernel, dim3(Q), dim3(VT), 0, (hipStream_t)stream, pair_score, pair_cells, pair_video, pair_ptr, gt_video, P, Q, n,
                       alpha, (long long*)out_video, out_score, out_count, pair_rank, weight, gt_rank);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_moment_reweight(void* stream, const float* score, const int32_t* count, const int32_t* pair_rank, const float* weight, int P,
                                    int k, int max_videos, float* out_score, int32_t* out_count)
{
    SMIN_REQUIRE(P >= 0 && k >= 1 && k <= VR_MAX_N);
    if (P == 0) return 0;
    SMIN_REQUIRE(score && count && pair_rank && weight && out_score && out_count);
    const size_t total = (size_t)P * k;
    SMIN_REQUIRE((total + VT - 1) / VT <= 0x7fffffffull);
    hipLaunchKernelGGL(moment_reweight_kernel, dim3((unsigned)((total + VT - 1) / VT)), dim3(VT), 0, (hipStream_t)stream, score, count, pair_rank, weight,
                       total, k, max_videos, out_score, out_count);
    SMIN_LAUNCH_CHECK();
    return 0;
}
