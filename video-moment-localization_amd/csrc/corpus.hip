// Corpus search (SMIN.search): Q queries against a bank of V videos.  The backbone's two encoders run once per
// video and once per query; the first place where a video and a query meet is the Hadamard product f = f_v * f_s (reference
// models.py:81), so a scored (video, query) pair starts here:
//   smin_pair_assemble  forms f, f_w, f_s of P pairs from the banks through two index lists, in one launch;
//   smin_corpus_topk    merges the pairs' top_moments lists into one ranked list per query across videos.
// Neither has a backward: the path only scores.
#include "common.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int CT = 256;                  // threads of a smin_corpus_topk workgroup
constexpr int CORPUS_MAX_K = 64;

// One float4 per thread over the P * (T + Nq + 1) * D4 output quads: row r of pair p is frame r of f (r < T), word r - T of f_w
// (r < T + Nq) or f_s.  The product is the one fp32 multiplication per element of video_enc_gate_kernel (video_encoder.hip); the
// gathers move bits.  Both indices are clamped before they form an address.
__global__ __launch_bounds__(256)
void pair_assemble_kernel(const float* __restrict__ fv, const float* __restrict__ fs_bank, const float* __restrict__ fw_bank,
                          const int* __restrict__ video_index, const int* __restrict__ query_index, int V, int Q, int T, int Nq, int D4,
                          size_t total, float* __restrict__ f, float* __restrict__ fw, float* __restrict__ fs)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int R = T + Nq + 1;
    const int d4 = (int)(idx % D4);
    const size_t pr = idx / D4;
    const size_t p = pr / R;
    const int r = (int)(pr - p * R);
    const size_t q = (size_t)min(max(query_index[p], 0), Q - 1);
    const float4 s = ldg4(fs_bank + (q * D4 + d4) * 4);
    if (r < T) {
        const size_t v = (size_t)min(max(video_index[p], 0), V - 1);
        stg4(f + ((p * T + r) * D4 + d4) * 4, f4mul(ldg4(fv + ((v * T + r) * D4 + d4) * 4), s));
    } else if (r < T + Nq) {
        const int w = r - T;
        stg4(fw + ((p * Nq + w) * D4 + d4) * 4, ldg4(fw_bank + ((q * Nq + w) * D4 + d4) * 4));
    } else {
        stg4(fs + (p * D4 + d4) * 4, s);
    }
}

// ---- merge across videos: one workgroup per query, K rounds of "the best candidate strictly after the previous pick" (a block
// argmax of order keys), as the cross-window merge of moments.hip without its suppression: no sort, no atomics, any pair count.
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t corpus_score_ord(float v)      // score_ord of moments.hip
{
    if (v == 0.f) v = 0.f;                                       // -0 -> +0
    const uint32_t u = __float_as_uint(v);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return o ? o : 1u;                                           // hi == 0 is "no candidate"
}

// Order key of a candidate, larger = earlier: (score, lower video, lower slot, lower pair ordinal within the query -- the last
// only separates two pairs of one query that name the same video).
struct Key { u64 hi, lo; };
__device__ __forceinline__ bool key_less(const Key& a, const Key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ Key make_key(float score, int video, int slot, long long w)
{
    Key k;
    k.hi = ((u64)corpus_score_ord(score) << 32) | (uint32_t)~((uint32_t)video ^ 0x80000000u);      // int32 ascending -> uint32 descending
    k.lo = ((u64)(uint32_t)(CORPUS_MAX_K - 1 - slot) << 56) | (u64)(0x00ffffffffffffffull - (u64)w);
    return k;
}

__device__ __forceinline__ Key block_max_key(Key v, Key* red)
{
    for (int o = 32; o >= 1; o >>= 1) {
        Key x;
        x.hi = __shfl_xor(v.hi, o); x.lo = __shfl_xor(v.lo, o);
        if (key_less(v, x)) v = x;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    Key m = red[0];
#pragma unroll
    for (int w = 1; w < CT / 64; ++w) if (key_less(m, red[w])) m = red[w];
    return m;
}

__global__ __launch_bounds__(CT)
void corpus_topk_kernel(const float* __restrict__ pair_score, const long long* __restrict__ pair_idx, const int* __restrict__ pair_count,
                        const int* __restrict__ pair_video, const int* __restrict__ pair_ptr, int kv, int K,
                        long long* __restrict__ out_video /* [Q][K] */, long long* __restrict__ out_idx /* [Q][K][2] */,
                        float* __restrict__ out_score /* [Q][K] */, int* __restrict__ out_count)
{
    __shared__ Key red[CT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const long long g0 = max(pair_ptr[b], 0);
    const long long g1 = max((long long)pair_ptr[b + 1], g0);
    const bool lists = pair_score && pair_idx && pair_count && pair_video;     // (NULL lists: no query may have a pair, none is read)
    const long long nslot = lists ? (g1 - g0) * kv : 0;          // candidate c = pair ordinal * kv + slot
    Key cursor; cursor.hi = ~0ull; cursor.lo = ~0ull;
    int nk = 0;
    for (; nk < K; ++nk) {
        Key best; best.hi = 0; best.lo = 0;
        for (long long c = t; c < nslot; c += CT) {
            const long long w = c / kv;
            const int slot = (int)(c - w * kv);
            const long long g = g0 + w;
            if (slot >= min(pair_count[g], kv)) continue;        // (a negative count lists nothing)
            const Key key = make_key(pair_score[g * kv + slot], pair_video[g], slot, w);
            if (!key_less(key, cursor) || !key_less(best, key)) continue;
            best = key;
        }
        best = block_max_key(best, red);
        if (best.hi == 0) break;                                 // the candidates ran out
        cursor = best;
        if (t == 0) {
            const long long w = (long long)(0x00ffffffffffffffull - (best.lo & 0x00ffffffffffffffull));
            const int slot = CORPUS_MAX_K - 1 - (int)(best.lo >> 56);
            const long long g = g0 + w, c = g * kv + slot;
            const size_t o = (size_t)b * K + nk;
            out_video[o] = pair_video[g];
            out_idx[2 * o] = pair_idx[2 * c]; out_idx[2 * o + 1] = pair_idx[2 * c + 1];
            out_score[o] = pair_score[c];
        }
        __syncthreads();
    }
    for (int r = nk + t; r < K; r += CT) {
        const size_t o = (size_t)b * K + r;
        out_video[o] = -1;
        out_idx[2 * o] = out_idx[2 * o + 1] = -1;
        out_score[o] = 0.f;
    }
    if (t == 0) out_count[b] = nk;
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" int smin_pair_assemble(void* stream, const float* fv, const float* fs_bank, const float* fw_bank, const int32_t* video_index,
                                  const int32_t* query_index, int P, int V, int Q, int T, int Nq, int D, float* f, float* fw, float* fs)
{
    SMIN_REQUIRE(D >= 4 && D % 4 == 0 && P >= 1 && V >= 1 && Q >= 1 && T >= 1 && Nq >= 1);
    SMIN_REQUIRE(fv != nullptr && fs_bank != nullptr && fw_bank != nullptr && video_index != nullptr && query_index != nullptr);
    SMIN_REQUIRE(f != nullptr && fw != nullptr && fs != nullptr);
    const size_t total = (size_t)P * ((size_t)T + Nq + 1) * (D / 4);
    SMIN_REQUIRE((total + 255) / 256 <= 0x7fffffffull);
    hipLaunchKernelGGL(pair_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fv, fs_bank, fw_bank, video_index,
                       query_index, V, Q, T, Nq, D / 4, total, f, fw, fs);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_corpus_topk(void* stream, const float* pair_score, const int64_t* pair_idx, const int32_t* pair_count, const int32_t* pair_video,
                                const int32_t* pair_ptr, int Q, int k_video, int K, int64_t* out_video, int64_t* out_idx, float* out_score,
                                int32_t* out_count)
{
    SMIN_REQUIRE(K >= 1 && K <= CORPUS_MAX_K && k_video >= 1 && k_video <= CORPUS_MAX_K && Q >= 0);
    if (Q == 0) return 0;
    SMIN_REQUIRE(pair_ptr != nullptr && out_video != nullptr && out_idx != nullptr && out_score != nullptr && out_count != nullptr);
    // (whether a query has pairs is known on the device only: with a NULL pair list the kernel reads none of the four and every query comes out empty)
    hipLaunchKernelGGL(corpus_topk_kernel, dim3(Q), dim3(CT), 0, (hipStream_t)stream, pair_score, (const long long*)pair_idx, pair_count, pair_video,
                       pair_ptr, k_video, K, (long long*)out_video, (long long*)out_idx, out_score, out_count);
    SMIN_LAUNCH_CHECK();
    return 0;
}
