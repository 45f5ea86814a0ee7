// What moments.hip (greedy hard NMS) and soft_nms.hip (Soft-NMS) must agree on bit for bit: a map's cells and their score, the
// order key of a cell, the IoU of two cells, the span of a window's cell in raw rows with the IoU of two spans, and the frame of the
// two merge kernels around their round loops.  One copy each.
#pragma once
#include "common.h"
#include "rank_order.h"

namespace smin {

constexpr int MOMENT_THREADS = 256;     // threads per workgroup (4 waves) of every kernel over these cells
constexpr int MOMENT_MAX_K = 64;
constexpr int MOMENT_MAX_B = 65535;     // the banded kernels put the sample in the grid's second dimension

struct Map {                            // one sample's inputs
    const float* pm; const float* ps; const float* pe; const uint8_t* mm; int L; int n;
};

// order key of a cell: the score's order word (rank_order.h's score_ord: 0 is "no cell") above 0x7fffffff - flat index
__device__ __forceinline__ u64 make_key(uint32_t o, int c) { return ((u64)o << 32) | (uint32_t)(0x7fffffff - c); }
__device__ __forceinline__ int key_cell(u64 k) { return 0x7fffffff - (int)(uint32_t)k; }

// score of cell c = (i, j): fp32, in this order, correctly rounded sqrtf
__device__ __forceinline__ float cell_score(const Map& m, int c, int i, int j) { return (m.pm[c] * sqrtf(m.ps[i])) * sqrtf(m.pe[j]); }

// IoU of two cells in clip units: one correctly rounded fp32 division
__device__ __forceinline__ float cell_iou(int i, int j, int i2, int j2)
{
    const int inter = max(0, min(j, j2) + 1 - max(i, i2)), uni = max(j, j2) + 1 - min(i, i2);
    return (float)inter / (float)uni;
}

// Visit cells lo + t, lo + t + MOMENT_THREADS, ... < hi in index order, with their row / column, without a division per cell.
template <typename F>
__device__ __forceinline__ void for_cells(const Map& m, int lo, int hi, F&& f)
{
    const int t = threadIdx.x, dq = MOMENT_THREADS / m.L, dr = MOMENT_THREADS % m.L;
    int c = lo + t, i = c / m.L, j = c - i * m.L;
    for (; c < hi; c += MOMENT_THREADS) {
        f(c, i, j);
        i += dq; j += dr;
        if (j >= m.L) { j -= m.L; ++i; }
    }
}

// ---- per-window top moments of long videos (smin_merge_window_moments and its soft form)
struct MergeIn {
    const long long* idx; const float* score; const int* count; const long long* start; const int* len;
    int G, T, L, kw;
};

// span in raw rows of cell (i, j) of window g (include/smin_hip.h, in this order, fp32; contraction off: a product and a sum are
// rounded one by one, never fused into an fma)
__device__ __forceinline__ void window_span(const MergeIn& in, int g, long long i, long long j, float& st, float& en)
{
#pragma clang fp contract(off)
    const long long s = in.start[g];
    const int n = in.len[g];
    const float u = (float)max(n, in.T) / (float)in.L;
    st = (float)s + (float)i * u;
    en = fminf((float)s + (float)(j + 1) * u, (float)(s + n));
}

__device__ __forceinline__ float span_iou(float st, float en, float st2, float en2)
{
    const float inter = fmaxf(0.f, fminf(en, en2) - fmaxf(st, st2));
    const float uni = fmaxf(en, en2) - fminf(st, st2);
    return inter / uni;
}

// ---- the frame of the two merge kernels (one workgroup per pair b, k rounds of one pick); none of these helpers synchronises
struct MergeOut {                       // [B][k] lists; raw_score: soft rules only, null in the hard merge
    float* __restrict__ span; float* __restrict__ score; float* __restrict__ raw_score;
    long long* __restrict__ window; long long* __restrict__ cell; int* __restrict__ count;
};

// pair b's first window and its candidate count, from pair_ptr[b], pair_ptr[b + 1] clamped into [0, G] and ascending
struct MergePair { long long g0; int nslot; };
__device__ __forceinline__ MergePair merge_pair(const MergeIn& in, const long long* __restrict__ pair_ptr, int b)
{
    const long long g0 = min(max(pair_ptr[b], 0LL), (long long)in.G);
    const long long g1 = min(max(pair_ptr[b + 1], g0), (long long)in.G);
    return {g0, (int)(g1 - g0) * in.kw};                         // (< 2^31: checked on the host)
}

// candidate q = window ordinal * kw + slot of a pair: the ordinal w, the window g, the flat index c into idx / score, and the
// slot, which holds a moment when slot < count[g]
struct MergeCand { int w, slot; long long g, c; };
__device__ __forceinline__ MergeCand merge_cand(const MergeIn& in, long long g0, int q)
{
    const int w = q / in.kw, slot = q - w * in.kw;
    const long long g = g0 + w;
    return {w, slot, g, g * in.kw + slot};
}
__device__ __forceinline__ void cand_span(const MergeIn& in, const MergeCand& x, float& st, float& en)
{
    window_span(in, (int)x.g, in.idx[2 * x.c], in.idx[2 * x.c + 1], st, en);
}

// one thread records candidate q as entry o = b * k + pick of the lists and returns its span.  With raw_score: score = v (the decayed
// score at pick time) and raw_score = the input score; without: score = the input score.
__device__ __forceinline__ void merge_record(const MergeIn& in, const MergeOut& out, long long g0, int q, size_t o, float v, float& st, float& en)
{
    const MergeCand x = merge_cand(in, g0, q);
    const long long i = in.idx[2 * x.c], j = in.idx[2 * x.c + 1];
    const float s = in.score[x.c];
    float s0, e0;
    window_span(in, (int)x.g, i, j, s0, e0);
    st = s0; en = e0;
    out.span[2 * o] = s0; out.span[2 * o + 1] = e0;
    out.score[o] = out.raw_score ? v : s;
    if (out.raw_score) out.raw_score[o] = s;
    out.window[o] = x.w;
    out.cell[2 * o] = i; out.cell[2 * o + 1] = j;
}

// the empty slots nk .. k of pair b (NaN span, score 0, window and cell -1) and its count
__device__ __forceinline__ void merge_finish(const MergeOut& out, int b, int k, int nk)
{
    for (int r = nk + threadIdx.x; r < k; r += MOMENT_THREADS) {
        const size_t o = (size_t)b * k + r;
        out.span[2 * o] = out.span[2 * o + 1] = __int_as_float(0x7fc00000);
        out.score[o] = 0.f;
        if (out.raw_score) out.raw_score[o] = 0.f;
        out.window[o] = -1;
        out.cell[2 * o] = out.cell[2 * o + 1] = -1;
    }
    if (threadIdx.x == 0) out.count[b] = nk;
}

// what both merge entry points require of their arguments; with B == 0 (nothing to launch) the pointers are not looked at
static inline bool merge_args_ok(const MergeIn& in, const void* pair_ptr, int B, int k, const MergeOut& out)
{
    if (k < 1 || k > MOMENT_MAX_K || in.kw < 1 || in.kw > MOMENT_MAX_K || in.G < 0 || B < 0 || in.T < 1 || in.L < 1) return false;
    if ((long long)in.G * in.kw >= 0x7fffffffLL) return false;
    if (B == 0) return true;
    if (!pair_ptr || !out.span || !out.score || !out.window || !out.cell || !out.count) return false;
    return in.G == 0 || (in.idx && in.score && in.count && in.start && in.len);
}

static inline size_t moment_align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline bool moment_args_ok(int B, int L, int k)
{
    return B >= 1 && B <= MOMENT_MAX_B && L >= 1 && (long long)L * L < 0x7fffffffLL && k >= 1 && k <= MOMENT_MAX_K;
}

}  // namespace smin
