// Corpus search (SMIN.search): Q queries against a bank of V videos.  The backbone's two encoders run once per
// video and once per query; the first place where a video and a query meet is the Hadamard product f = f_v * f_s (reference
// models.py:81), so a scored (video, query) pair starts here:
//   smin_pair_assemble  forms f, f_w, f_s of P pairs from the banks through two index lists, in one launch;
//   smin_corpus_topk    merges the pairs' top_moments lists into one ranked list per query across videos;
//   smin_search_merge   merges up to 16 such ranked lists of disjoint video shards into one: the same K-round
//                       selection (topk_rounds) over another way of reading candidate c, so a merge of the shards' lists is the list
//                       smin_corpus_topk gives on the whole corpus.
// smin_pair_assemble has an adjoint, which is what lets a model train through shared banks:
//   smin_pair_assemble_bwd  sums the pairs' gradients of f, f_w, f_s back onto the videos and queries they came from, through the
//                           pairs grouped by video and by query (two CSR lists from the host): no atomics, a fixed order.
// The two merges have no backward.
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

// ---- the adjoint of pair_assemble_kernel.  df [P][T][D] is by far the largest operand and is read ONCE: a thread owns one float4
// column d4 of BWD_TC consecutive frames of one video v and walks v's pairs in segment order; per pair it reads its BWD_TC quads of df,
// adds df * fs_bank[qi[p]] to the frames' running sums (dfv, kept in registers) and writes the pair's partial dot with its own quads of
// fv (registers as well, so fv is read once in all) to part [P][TC][D], TC = ceil(T / BWD_TC).  pair_bwd_query_kernel then sums, per
// query, its pairs' partials and dfs in a fixed order (below).  The remaining threads of the first launch sum dfw.
// Every value read from a list is clamped before it forms an address.
constexpr int BWD_TC = 4;

__device__ __forceinline__ float4 f4fma(float4 a, float4 b, float4 c)
{
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ void segment(const int* __restrict__ ptr, int g, int P, int& s0, int& s1)
{
    s0 = min(max(ptr[g], 0), P);
    s1 = min(max(ptr[g + 1], s0), P);
}

__global__ __launch_bounds__(256)
void pair_bwd_video_kernel(const float* __restrict__ df, const float* __restrict__ dfw, const float* __restrict__ fv, const float* __restrict__ fs_bank,
                           const int* __restrict__ query_index, const int* __restrict__ v_ptr, const int* __restrict__ v_pairs,
                           const int* __restrict__ q_ptr, const int* __restrict__ q_pairs, int P, int V, int Q, int T, int TC, int Nq, int D4,
                           size_t n_video, size_t total, float* __restrict__ dfv, float* __restrict__ dfw_bank, float* __restrict__ part)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (idx < n_video) {                                         // (v, frame chunk c, d4)
        const int d4 = (int)(idx % D4);
        const size_t vc = idx / D4;
        const size_t v = vc / TC;
        const int c = (int)(vc - v * TC), t0 = c * BWD_TC;
        float4 x[BWD_TC], acc[BWD_TC];
#pragma unroll
        for (int j = 0; j < BWD_TC; ++j) {
            x[j] = t0 + j < T ? ldg4(fv + ((v * T + t0 + j) * D4 + d4) * 4) : zero;
            acc[j] = zero;
        }
        int s0, s1;
        segment(v_ptr, (int)v, P, s0, s1);
        for (int s = s0; s < s1; ++s) {
            const size_t p = (size_t)min(max(v_pairs[s], 0), P - 1);
            const size_t q = (size_t)min(max(query_index[p], 0), Q - 1);
            const float4 g = ldg4(fs_bank + (q * D4 + d4) * 4);
            float4 dot = zero;
#pragma unroll
            for (int j = 0; j < BWD_TC; ++j) {
                if (t0 + j < T) {
                    const float4 d = ldg4(df + ((p * T + t0 + j) * D4 + d4) * 4);
                    acc[j] = f4fma(d, g, acc[j]);
                    dot = f4fma(d, x[j], dot);
                }
            }
            stg4(part + ((p * TC + c) * D4 + d4) * 4, dot);
        }
#pragma unroll
        for (int j = 0; j < BWD_TC; ++j)
            if (t0 + j < T) stg4(dfv + ((v * T + t0 + j) * D4 + d4) * 4, acc[j]);
    } else {                                                     // (q, word w, d4)
        const size_t i = idx - n_video;
        const int d4 = (int)(i % D4);
        const size_t qw = i / D4;
        const size_t q = qw / Nq;
        const int w = (int)(qw - q * Nq);
        float4 acc = zero;
        int s0, s1;
        segment(q_ptr, (int)q, P, s0, s1);
        for (int s = s0; s < s1; ++s) {
            const size_t p = (size_t)min(max(q_pairs[s], 0), P - 1);
            acc = f4add(acc, dfw ? ldg4(dfw + ((p * Nq + w) * D4 + d4) * 4) : zero);
        }
        stg4(dfw_bank + ((q * Nq + w) * D4 + d4) * 4, acc);
    }
}

// One workgroup per (query, tile of BWD_QD quads): BWD_QJ lanes share the chunks of a pair, lane j taking c = j, j + BWD_QJ, ... (the
// loads of a lane are independent: a single thread walking all chunks of all pairs is one latency chain).  Lane j sums over the
// segment's pairs in list order, within a pair over its chunks in ascending c; dfs[p] joins lane 0; the lanes are then added in
// ascending j.  A fixed order, a function of the arguments only.
constexpr int BWD_QD = 32, BWD_QJ = 8;

__global__ __launch_bounds__(BWD_QD * BWD_QJ)
void pair_bwd_query_kernel(const float* __restrict__ dfs, const float* __restrict__ part, const int* __restrict__ q_ptr, const int* __restrict__ q_pairs,
                           int P, int TC, int D4, float* __restrict__ dfs_bank)
{
    __shared__ float4 red[BWD_QJ][BWD_QD];
    const int lane = threadIdx.x % BWD_QD, j = threadIdx.x / BWD_QD;
    const int d4 = blockIdx.x * BWD_QD + lane;
    const size_t q = blockIdx.y;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc = zero;
    if (d4 < D4) {
        int s0, s1;
        segment(q_ptr, (int)q, P, s0, s1);
        for (int s = s0; s < s1; ++s) {
            const size_t p = (size_t)min(max(q_pairs[s], 0), P - 1);
            if (j == 0) acc = f4add(acc, dfs ? ldg4(dfs + (p * D4 + d4) * 4) : zero);
            for (int c = j; c < TC; c += BWD_QJ) acc = f4add(acc, ldg4(part + ((p * TC + c) * D4 + d4) * 4));
        }
    }
    red[j][lane] = acc;
    __syncthreads();
    if (j == 0 && d4 < D4) {
#pragma unroll
        for (int k = 1; k < BWD_QJ; ++k) acc = f4add(acc, red[k][lane]);
        stg4(dfs_bank + (q * D4 + d4) * 4, acc);
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

// The K rounds over a source of candidates.  Src::read(c, slot, w, score, video) says whether candidate c < ncand exists and gives
// its key parts (slot < 64 and w < 2^56: the key's two low fields, lower first); Src::emit(slot, w, ...) copies the picked one out.
template <class Src>
__device__ __forceinline__ void topk_rounds(const Src& src, long long ncand, int K, long long* __restrict__ out_video /* [Q][K] */,
                                            long long* __restrict__ out_idx /* [Q][K][2] */, float* __restrict__ out_score /* [Q][K] */,
                                            int* __restrict__ out_count)
{
    __shared__ Key red[CT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    Key cursor; cursor.hi = ~0ull; cursor.lo = ~0ull;
    int nk = 0;
    for (; nk < K; ++nk) {
        Key best; best.hi = 0; best.lo = 0;
        for (long long c = t; c < ncand; c += CT) {
            int slot, video; long long w; float score;
            if (!src.read(c, slot, w, score, video)) continue;
            const Key key = make_key(score, video, slot, w);
            if (!key_less(key, cursor) || !key_less(best, key)) continue;
            best = key;
        }
        best = block_max_key(best, red);
        if (best.hi == 0) break;                                 // the candidates ran out
        cursor = best;
        if (t == 0) {
            const long long w = (long long)(0x00ffffffffffffffull - (best.lo & 0x00ffffffffffffffull));
            const int slot = CORPUS_MAX_K - 1 - (int)(best.lo >> 56);
            const size_t o = (size_t)b * K + nk;
            src.emit(slot, w, out_video + o, out_idx + 2 * o, out_score + o);
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

// smin_corpus_topk's candidates: c = pair ordinal * kv + slot over the query's pairs g0 .. ; key parts (slot, pair ordinal)
struct PairLists {
    const float* score; const long long* idx; const int* count; const int* video;
    long long g0; int kv;
    __device__ __forceinline__ bool read(long long c, int& slot, long long& w, float& sc, int& vid) const
    {
        w = c / kv;
        slot = (int)(c - w * kv);
        const long long g = g0 + w;
        if (slot >= min(count[g], kv)) return false;             // (a negative count lists nothing)
        sc = score[g * kv + slot];
        vid = video[g];
        return true;
    }
    __device__ __forceinline__ void emit(int slot, long long w, long long* ov, long long* oi, float* os) const
    {
        const long long g = g0 + w, c = g * kv + slot;
        *ov = video[g];
        oi[0] = idx[2 * c]; oi[1] = idx[2 * c + 1];
        *os = score[c];
    }
};

__global__ __launch_bounds__(CT)
void corpus_topk_kernel(const float* __restrict__ pair_score, const long long* __restrict__ pair_idx, const int* __restrict__ pair_count,
                        const int* __restrict__ pair_video, const int* __restrict__ pair_ptr, int kv, int K,
                        long long* __restrict__ out_video, long long* __restrict__ out_idx, float* __restrict__ out_score, int* __restrict__ out_count)
{
    const int b = blockIdx.x;
    const long long g0 = max(pair_ptr[b], 0);
    const long long g1 = max((long long)pair_ptr[b + 1], g0);
    const bool lists = pair_score && pair_idx && pair_count && pair_video;     // (NULL lists: no query may have a pair, none is read)
    const PairLists src{pair_score, pair_idx, pair_count, pair_video, g0, kv};
    topk_rounds(src, lists ? (g1 - g0) * kv : 0, K, out_video, out_idx, out_score, out_count);
}

// smin_search_merge's candidates: S ranked lists of k[s] slots per query, c = base[s] + p (base: the exclusive prefix of k); key
// parts (list s <= 15, position p).  Passed to the kernel by value: the host tables need no copy of their own.
constexpr int MERGE_MAX_S = 16;
struct RankedTables {
    const long long* video[MERGE_MAX_S]; const long long* idx[MERGE_MAX_S]; const float* score[MERGE_MAX_S]; const int* count[MERGE_MAX_S];
    long long offset[MERGE_MAX_S];
    int k[MERGE_MAX_S], base[MERGE_MAX_S + 1], S;
};
struct RankedLists {
    const RankedTables& tb; long long q;
    __device__ __forceinline__ bool read(long long c, int& slot, long long& w, float& sc, int& vid) const
    {
        int s = 0;
        while (s + 1 < tb.S && c >= tb.base[s + 1]) ++s;
        const int p = (int)c - tb.base[s], ks = tb.k[s];
        if (p >= min(tb.count[s][q], ks)) return false;          // behind the count: never read
        slot = s; w = p;
        sc = tb.score[s][q * ks + p];
        vid = (int)(tb.video[s][q * ks + p] + tb.offset[s]);     // the key's field: global ids lie in [0, 2^31)
        return true;
    }
    __device__ __forceinline__ void emit(int s, long long p, long long* ov, long long* oi, float* os) const
    {
        const long long c = q * tb.k[s] + p;
        *ov = tb.video[s][c] + tb.offset[s];
        oi[0] = tb.idx[s][2 * c]; oi[1] = tb.idx[s][2 * c + 1];
        *os = tb.score[s][c];
    }
};

__global__ __launch_bounds__(CT)
void search_merge_kernel(const RankedTables tb, int K, long long* __restrict__ out_video, long long* __restrict__ out_idx,
                         float* __restrict__ out_score, int* __restrict__ out_count)
{
    const RankedLists src{tb, (long long)blockIdx.x};
    topk_rounds(src, tb.base[tb.S], K, out_video, out_idx, out_score, out_count);
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

extern "C" size_t smin_pair_assemble_bwd_workspace_bytes(int P, int T, int D)
{
    if (P < 1 || T < 1 || D < 4) return 0;
    return (size_t)P * ((T + BWD_TC - 1) / BWD_TC) * D * sizeof(float);
}

extern "C" int smin_pair_assemble_bwd(void* stream, const float* df, const float* dfw, const float* dfs, const float* fv, const float* fs_bank,
                                      const int32_t* video_index, const int32_t* query_index, const int32_t* v_ptr, const int32_t* v_pairs,
                                      const int32_t* q_ptr, const int32_t* q_pairs, int P, int V, int Q, int T, int Nq, int D, float* dfv,
                                      float* dfw_bank, float* dfs_bank, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(D >= 4 && D % 4 == 0 && P >= 1 && V >= 1 && Q >= 1 && T >= 1 && Nq >= 1);
    SMIN_REQUIRE(df != nullptr && fv != nullptr && fs_bank != nullptr && video_index != nullptr && query_index != nullptr);
    SMIN_REQUIRE(v_ptr != nullptr && v_pairs != nullptr && q_ptr != nullptr && q_pairs != nullptr);
    SMIN_REQUIRE(dfv != nullptr && dfw_bank != nullptr && dfs_bank != nullptr);
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= smin_pair_assemble_bwd_workspace_bytes(P, T, D));
    const int D4 = D / 4, TC = (T + BWD_TC - 1) / BWD_TC;
    const size_t n_video = (size_t)V * TC * D4, total = n_video + (size_t)Q * Nq * D4;
    SMIN_REQUIRE((total + 255) / 256 <= 0x7fffffffull && (size_t)P * TC <= 0x7fffffffull && Q <= 65535);
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(pair_bwd_video_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, df, dfw, fv, fs_bank, query_index, v_ptr,
                       v_pairs, q_ptr, q_pairs, P, V, Q, T, TC, Nq, D4, n_video, total, dfv, dfw_bank, part);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_bwd_query_kernel, dim3((unsigned)((D4 + BWD_QD - 1) / BWD_QD), (unsigned)Q), dim3(BWD_QD * BWD_QJ), 0, (hipStream_t)stream, dfs, part, q_ptr,
                       q_pairs, P, TC, D4, dfs_bank);
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

extern "C" int smin_search_merge(void* stream, int S, const int64_t* const* video, const int64_t* const* idx, const float* const* score,
                                 const int32_t* const* count, const int32_t* k_list, const int64_t* video_offset, int Q, int K,
                                 int64_t* out_video, int64_t* out_idx, float* out_score, int32_t* out_count)
{
    SMIN_REQUIRE(S >= 1 && S <= MERGE_MAX_S && K >= 1 && K <= CORPUS_MAX_K && Q >= 0);
    RankedTables tb{};
    tb.S = S;
    if (k_list) {
        for (int s = 0; s < S; ++s) {
            SMIN_REQUIRE(k_list[s] >= 1 && k_list[s] <= CORPUS_MAX_K);
            tb.k[s] = k_list[s];
            tb.base[s + 1] = tb.base[s] + k_list[s];
        }
    }
    if (Q == 0) return 0;
    SMIN_REQUIRE(video != nullptr && idx != nullptr && score != nullptr && count != nullptr && k_list != nullptr && video_offset != nullptr);
    SMIN_REQUIRE(out_video != nullptr && out_idx != nullptr && out_score != nullptr && out_count != nullptr);
    for (int s = 0; s < S; ++s) {
        SMIN_REQUIRE(video[s] != nullptr && idx[s] != nullptr && score[s] != nullptr && count[s] != nullptr);
        SMIN_REQUIRE(video_offset[s] >= 0 && video_offset[s] <= 0x7fffffffll);
        const void* in[4] = {video[s], idx[s], score[s], count[s]};
        for (const void* p : in)                                 // the rounds read the lists while thread 0 writes the result
            SMIN_REQUIRE(p != (const void*)out_video && p != (const void*)out_idx && p != (const void*)out_score && p != (const void*)out_count);
        tb.video[s] = (const long long*)video[s]; tb.idx[s] = (const long long*)idx[s]; tb.score[s] = score[s]; tb.count[s] = count[s];
        tb.offset[s] = video_offset[s];
    }
    hipLaunchKernelGGL(search_merge_kernel, dim3(Q), dim3(CT), 0, (hipStream_t)stream, tb, K, (long long*)out_video, (long long*)out_idx, out_score,
                       out_count);
    SMIN_LAUNCH_CHECK();
    return 0;
}
