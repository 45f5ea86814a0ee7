// What every ranking kernel of the library must agree on bit for bit -- the order word of a score and of a (score, video) candidate --
// and the reductions of a 256-thread workgroup (four waves) they are built from: one copy each, so top_moments' lists, the corpus
// merges, smin_video_rank and the prefilter's fold cannot drift apart, and a sharded search keeps matching the unsharded one.
#pragma once
#include "common.h"

namespace smin {

typedef unsigned long long u64;

// ---- order words: larger = earlier
// A score's fp32 bits as an unsigned total order.  -0 counts as +0; 0 is reserved for "nothing" (only -NaN 0xffffffff would map there).
__device__ __forceinline__ uint32_t score_ord(float v)
{
    if (v == 0.f) v = 0.f;                                       // -0 -> +0
    const uint32_t u = __float_as_uint(v);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return o ? o : 1u;
}
__device__ __forceinline__ float ord_score(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// the lower video first: int32 ascending -> uint32 descending
__device__ __forceinline__ uint32_t video_ord(int video) { return ~((uint32_t)video ^ 0x80000000u); }
// (score, then the lower video): never 0
__device__ __forceinline__ u64 video_word(float score, int video) { return ((u64)score_ord(score) << 32) | video_ord(video); }

// ---- a workgroup of 256 threads: a butterfly inside each wave, one LDS word per wave (red: 4 words), then the four waves.  Every
// thread gets the result; the leading barrier lets a kernel call them back to back on one `red` (and publishes its earlier LDS stores).
__device__ __forceinline__ int block_sum(int v, int* red)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ int block_min(int v, int* red)
{
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}
__device__ __forceinline__ u64 block_max(u64 v, u64* red)
{
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const u64 a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}
// fp32 sum: common.h's DPP wave_sum, then the four waves' totals as (w0 + w1) + (w2 + w3) -- one sequence of additions, so the loss
// and the pair pooling (pair_pool.h) round alike.  A __shfl_xor butterfly is another tree of additions: never swap one for the other.
__device__ __forceinline__ float block_sum(float v, float* red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// exclusive prefix of a 0/1 flag over the workgroup's threads in ascending order, and its total
__device__ __forceinline__ int block_scan_flag(bool flag, int* red, int& total)
{
    const u64 b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();                                             // (the previous scan's reads of red are done)
    if (lane == 0) red[wave] = __popcll(b);
    __syncthreads();
    int base = 0;
    for (int k = 0; k < 4; ++k) base += k < wave ? red[k] : 0;
    total = (red[0] + red[1]) + (red[2] + red[3]);
    return base + before;
}
// exclusive prefix of a non-negative 64-bit count over the workgroup's threads in ascending order, and its total: a shift-and-add scan
// inside each wave, one LDS word per wave (red: 4 words), then the waves in front
__device__ __forceinline__ long long block_scan_count(long long v, long long* red, long long& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    __syncthreads();                                             // (the previous scan's reads of red are done)
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    long long base = 0;
    for (int k = 0; k < 4; ++k) base += k < wave ? red[k] : 0;
    total = (red[0] + red[1]) + (red[2] + red[3]);
    return base + (incl - v);
}
// fp64 sum in a fixed order -- the butterfly, then the four wave sums as (w0 + w1) + (w2 + w3), no contraction --; valid in thread 0.
// No leading barrier: a kernel calls it once per `red`.
__device__ __forceinline__ double block_sum_f64_fixed(double acc, double* red)
{
#pragma clang fp contract(off)
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace smin
