// The pooling of one (video, query) pair's cells into its pair score, shared by the contrastive loss (pair_rank.hip)
// and the video ranking of corpus search (video_rank.hip): one copy of the device code, so both give the same bits.
//   cell score    f[p,i,j] = (pm[p,i,j] * sqrt(max(ps[p,i], 1e-12))) * sqrt(max(pe[p,j], 1e-12))        (top_moments' order)
//   pair score    s_p = m_p + tau * log( sum_valid exp((f - m_p) / tau) / n_p ),  m_p = max_valid f;  n_p == 0: s_p = 0
#pragma once
#include <cmath>

#include "common.h"
#include "rank_order.h"

namespace smin {

constexpr float RANK_CLAMP = 1e-12f;          // under the square roots, as torch.clamp_min: the derivative stays finite
constexpr int RANK_MAX_L = 4096;              // L * L cells are counted in fp32: exact up to 2^24

__device__ __forceinline__ float rank_root(float x) { return sqrtf(fmaxf(x, RANK_CLAMP)); }
// d sqrt(max(x, c)) / dx with clamp_min's gradient (passes where x >= c)
__device__ __forceinline__ float rank_root_grad(float x, float root) { return x >= RANK_CLAMP ? 0.5f / root : 0.f; }
__device__ __forceinline__ float rank_cell(float pm, float a, float b) { return (pm * a) * b; }
__device__ __forceinline__ float rank_exp(float f, float m, float tau) { return expf((f - m) / tau); }

__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    v = fmaxf(v, __shfl_xor(v, 2));
    v = fmaxf(v, __shfl_xor(v, 4));
    v = fmaxf(v, __shfl_xor(v, 8));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}
__device__ __forceinline__ float rank_block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

static inline bool rank_temperature(float v) { return std::isfinite(v) && v > 0.f; }

// What a workgroup of 256 finds of pair p's map, the same in every thread: m = the maximum over the valid cells (0 without one), sum =
// sum_valid exp((f - m) / tau) (0 without one), cnt = the number of valid cells, score = s_p.
struct PairPool { float m, sum, cnt, score; };

// Thread t takes cells t, t + 256, ... of the row-major map in ascending order; the maximum first, then the sum.  red: 4 floats of LDS.
__device__ __forceinline__ PairPool pair_pool_cells(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                                                    const uint8_t* __restrict__ mm, int p, int L, float tau, float* red)
{
    const int t = threadIdx.x;
    const size_t map = (size_t)p * L * L, row = (size_t)p * L;
    const int cells = L * L, di = 256 / L, dj = 256 % L;
    float mx = -INFINITY, cnt = 0.f;
    for (int k = t, i = t / L, j = t % L; k < cells; k += 256) {
        if (mm[map + k]) {
            mx = fmaxf(mx, rank_cell(pm[map + k], rank_root(ps[row + i]), rank_root(pe[row + j])));
            cnt += 1.f;
        }
        i += di; j += dj;
        if (j >= L) { j -= L; ++i; }
    }
    mx = rank_block_max(mx, red);
    cnt = block_sum(cnt, red);
    const float m = cnt > 0.f ? mx : 0.f;
    float sum = 0.f;
    for (int k = t, i = t / L, j = t % L; k < cells; k += 256) {
        if (mm[map + k]) sum += rank_exp(rank_cell(pm[map + k], rank_root(ps[row + i]), rank_root(pe[row + j])), m, tau);
        i += di; j += dj;
        if (j >= L) { j -= L; ++i; }
    }
    sum = block_sum(sum, red);
    PairPool r;
    r.m = m;
    r.sum = cnt > 0.f ? sum : 0.f;
    r.cnt = cnt;
    r.score = cnt > 0.f ? m + tau * logf(sum / cnt) : 0.f;
    return r;
}

}  // namespace smin
