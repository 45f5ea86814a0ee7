// The sort both backward passes of smin_embed_tokens start from (sampling.hip: the dense table gradient; row_sparse.hip: the compact one).
#pragma once
#include "common.h"

namespace smin {

constexpr int EMBED_BWD_MAX = 4096;      // positions B * Nq sorted in LDS (32 KB of keys)

// s[0 .. np) (np = n rounded up to a power of two, np <= EMBED_BWD_MAX) = the keys (id << 32 | position) of tokens[0 .. n) sorted ascending
// (bitonic sort in LDS, the whole workgroup); positions with an id outside [0, V) are given the largest key, ~0, and sort to the end.
// Equal ids end up adjacent, in ascending position order.  Ends with a barrier: every thread may read s.
__device__ __forceinline__ void embed_sort_keys(const int* __restrict__ tokens, int n, int V, unsigned long long* s)
{
    int np = 1;
    while (np < n) np <<= 1;
    for (int i = threadIdx.x; i < np; i += blockDim.x) {
        unsigned long long k = ~0ull;
        if (i < n) {
            const int id = tokens[i];
            if (id >= 0 && id < V) k = ((unsigned long long)(unsigned)id << 32) | (unsigned)i;
        }
        s[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < np; i += blockDim.x) {
                const int partner = i ^ stride;
                if (partner > i) {
                    const bool up = (i & size) == 0;
                    const unsigned long long a = s[i], c = s[partner];
                    if ((a > c) == up) { s[i] = c; s[partner] = a; }
                }
            }
            __syncthreads();
        }
}

}  // namespace smin
