// What moments.hip (greedy hard NMS) and soft_nms.hip (Soft-NMS) must agree on bit for bit: a map's cells and their score, the
// order key of a cell, the IoU of two cells, and the span of a window's cell in raw rows with the IoU of two spans.  One copy each.
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

static inline size_t moment_align256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline bool moment_args_ok(int B, int L, int k)
{
    return B >= 1 && B <= MOMENT_MAX_B && L >= 1 && (long long)L * L < 0x7fffffffLL && k >= 1 && k <= MOMENT_MAX_K;
}

}  // namespace smin
