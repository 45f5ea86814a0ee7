// Corpus search (SMIN.search): Q queries against a bank of V videos.  The backbone's two encoders run once per
// video and once per query; the first place where a video and a query meet is the Hadamard product f = f_v * f_s (reference
// models.py:81), so a scored (video, query) pair starts here:
//   smin_pair_assemble  forms f, f_w, f_s of P pairs from the banks through two index lists, in one launch;
//   smin_corpus_topk    merges the pairs' top_moments lists into one ranked list per query across videos;
//   smin_search_merge   merges up to 16 such ranked lists of disjoint video shards into one: the same K-round
//                       selection (topk_rounds) over another way of reading candidate c, so a merge of the shards' lists is the list
//                       smin_corpus_topk gives on the whole corpus;
//   smin_corpus_span_topk  ranks, per query, the span-valued moments of its videos (smin_merge_window_moments' lists of a bank of
//                       windows over long videos): the same rounds over the same key, five fields per entry;
//   smin_span_search_merge  merges up to 16 such span lists of shards of whole videos into one: the same order,
//                       found without the rounds -- the lists are sorted, so each candidate's rank is a sum of binary searches;
//   smin_search_merge_weighted / smin_span_search_merge_weighted  merge shard lists that carry their unweighted scores, under the
//                       video weights and ranks of the whole corpus: the lists are not sorted in that order, so
//                       each candidate counts the order words ahead of it.
// What an entry holds beside video and score (IdxFields: the clips; SpanFields: span, window, cell) is one trait for all six: their
// tables (ListTables), their output (ListOut), the host's checks (fill_tables) and the two group kernels are written once over it.
// smin_pair_assemble has an adjoint, which is what lets a model train through shared banks:
//   smin_pair_assemble_bwd  sums the pairs' gradients of f, f_w, f_s back onto the videos and queries they came from, through the
//                           pairs grouped by video and by query (two CSR lists from the host): no atomics, a fixed order.
// The merges have no backward.
// The training-side counterpart of the search:
//   smin_mine_pairs         picks, per query, its own video and the N highest-scoring wrong ones -- topk_rounds over a third way of
//                           reading candidate c, a row of pair scores without the query's own video -- and groups the picked pairs by
//                           video and by query on the device: the pair plan smin_pair_assemble_bwd reads, with no host in between.
#include "common.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int CT = 256;                  // threads of a smin_corpus_topk workgroup
static_assert(CT == 256, "rank_order.h's block helpers are written for four waves");
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
// Order key of a candidate, larger = earlier: (score, lower video, lower slot, lower pair ordinal within the query -- the last
// only separates two pairs of one query that name the same video).  hi is rank_order.h's video_word: hi == 0 is "no candidate".
struct Key { u64 hi, lo; };
__device__ __forceinline__ bool key_less(const Key& a, const Key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ Key make_key(float score, int video, int slot, long long w)
{
    Key k;
    k.hi = video_word(score, video);
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
// its key parts (slot < 64 and w < 2^56: the key's two low fields, lower first); Src::emit(r, slot, w) copies the r-th pick out, to
// wherever the source keeps its result.  Returns the number of picks (< K when the candidates ran out), the same in every thread.
template <class Src>
__device__ __forceinline__ int topk_rounds(const Src& src, long long ncand, int K)
{
    __shared__ Key red[CT / 64];
    const int t = threadIdx.x;
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
            src.emit(nk, slot, w);
        }
        __syncthreads();
    }
    return nk;
}

// What an entry of a ranked list holds beside video and score -- F::In the tables of a list, F::Out the output's, with move() and
// clear() (the empty pattern), and in(), which fills an In from the host's F::N table pointers -- is the parameter of everything below.
// An output may not be an input, but the compiler cannot know that of pointers inside a struct: whoever moves an entry reads all of
// it before the first store, so the loads go out together.
struct IdxFields {                           // SMIN.search: the moment's clips
    static constexpr int N = 1;
    struct In {
        const long long* idx;
        __device__ __forceinline__ bool present() const { return idx != nullptr; }
    };
    struct Out {
        long long* idx /* [Q][K][2] */;
        __device__ __forceinline__ void move(size_t o, const In& in, long long i) const
        {
            const long long a = in.idx[2 * i], b = in.idx[2 * i + 1];
            idx[2 * o] = a; idx[2 * o + 1] = b;
        }
        __device__ __forceinline__ void clear(size_t o) const { idx[2 * o] = idx[2 * o + 1] = -1; }
    };
    static In in(const void* const* p) { return In{(const long long*)p[0]}; }
};
struct SpanFields {                          // SMIN.search_windows: smin_merge_window_moments' span in raw rows, window and cell
    static constexpr int N = 3;
    struct In {
        const float* span; const long long* window; const long long* cell;
        __device__ __forceinline__ bool present() const { return span != nullptr && window != nullptr && cell != nullptr; }
    };
    struct Out {
        float* span /* [Q][K][2] */; long long* window /* [Q][K] */; long long* cell /* [Q][K][2] */;
        __device__ __forceinline__ void move(size_t o, const In& in, long long i) const
        {
            const float s0 = in.span[2 * i], s1 = in.span[2 * i + 1];                            // plain moves: the bits leave as they came
            const long long w = in.window[i], c0 = in.cell[2 * i], c1 = in.cell[2 * i + 1];
            span[2 * o] = s0; span[2 * o + 1] = s1;
            window[o] = w;
            cell[2 * o] = c0; cell[2 * o + 1] = c1;
        }
        __device__ __forceinline__ void clear(size_t o) const
        {
            span[2 * o] = span[2 * o + 1] = __uint_as_float(0x7fc00000u);
            window[o] = -1;
            cell[2 * o] = cell[2 * o + 1] = -1;
        }
    };
    static In in(const void* const* p) { return In{(const float*)p[0], (const long long*)p[1], (const long long*)p[2]}; }
};

// Where a kernel leaves query blockIdx.x's ranked list: entry r of K, and the empty slots behind the nk listed ones.
template <class F>
struct ListOut {
    long long* video /* [Q][K] */; float* score /* [Q][K] */; int* count /* [Q] */;
    typename F::Out f;
    int K;
    __device__ __forceinline__ size_t at(int r) const { return (size_t)blockIdx.x * K + r; }
    __device__ __forceinline__ void clear(size_t o) const
    {
        video[o] = -1;
        score[o] = 0.f;
        f.clear(o);
    }
    __device__ __forceinline__ void finish(int nk) const
    {
        for (int r = nk + threadIdx.x; r < K; r += CT) clear(at(r));
        if (threadIdx.x == 0) count[blockIdx.x] = nk;
    }
};

// smin_corpus_topk's and smin_corpus_span_topk's candidates: c = group ordinal * kv + slot over the query's pairs (groups) g0 .. ; key
// parts (slot, group ordinal)
template <class F>
struct GroupLists {
    const float* score; const int* count; const int* video; typename F::In in;
    long long g0; int kv; ListOut<F> out;
    __device__ __forceinline__ bool read(long long c, int& slot, long long& w, float& sc, int& vid) const
    {
        w = c / kv;
        slot = (int)(c - w * kv);
        const long long g = g0 + w;
        if (slot >= min(count[g], kv)) return false;             // behind the count (a negative one lists nothing): never read
        sc = score[g * kv + slot];
        vid = video[g];
        return true;
    }
    __device__ __forceinline__ void emit(int r, int slot, long long w) const
    {
        const long long g = g0 + w, c = g * kv + slot;
        const size_t o = out.at(r);
        const int v = video[g];
        const float sc = score[c];
        out.f.move(o, in, c);
        out.video[o] = v;
        out.score[o] = sc;
    }
};

template <class F>
__global__ __launch_bounds__(CT)
void group_topk_kernel(const float* __restrict__ score, const int* __restrict__ count, const int* __restrict__ group_video,
                       const int* __restrict__ group_ptr, const typename F::In in, int kv, const ListOut<F> out)
{
    const int b = blockIdx.x;
    const long long g0 = max(group_ptr[b], 0);
    const long long g1 = max((long long)group_ptr[b + 1], g0);
    const bool lists = score && count && group_video && in.present();    // (NULL lists: no query may have a group, none is read)
    const GroupLists<F> src{score, count, group_video, in, g0, kv, out};
    out.finish(topk_rounds(src, lists ? (g1 - g0) * kv : 0, out.K));
}

// The tables of S <= 16 ranked lists of k[s] slots per query, from disjoint video shards: candidate c = base[s] + p (base: the exclusive
// prefix of k), its global video = video + offset[s].  Passed to a kernel by value: the host tables need no copy of their own.
constexpr int MERGE_MAX_S = 16;
template <class F>
struct ListTables {
    const long long* video[MERGE_MAX_S]; const float* score[MERGE_MAX_S]; const int* count[MERGE_MAX_S]; typename F::In in[MERGE_MAX_S];
    long long offset[MERGE_MAX_S];
    int k[MERGE_MAX_S], base[MERGE_MAX_S + 1], S;
};

// smin_search_merge's candidates: key parts (list s <= 15, position p)
struct RankedLists {
    const ListTables<IdxFields>& tb; long long q; ListOut<IdxFields> out;
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
    __device__ __forceinline__ void emit(int r, int s, long long p) const
    {
        const long long c = q * tb.k[s] + p;
        const size_t o = out.at(r);
        const long long v = tb.video[s][c] + tb.offset[s];
        const float sc = tb.score[s][c];
        out.f.move(o, tb.in[s], c);
        out.video[o] = v;
        out.score[o] = sc;
    }
};

__global__ __launch_bounds__(CT)
void search_merge_kernel(const ListTables<IdxFields> tb, const ListOut<IdxFields> out)
{
    const RankedLists src{tb, (long long)blockIdx.x, out};
    out.finish(topk_rounds(src, tb.base[tb.S], out.K));
}

// smin_span_search_merge: S ranked span lists of disjoint video shards into one, in ONE pass instead of K rounds.
// Each list is sorted, so a candidate's place in the merge is its own position plus, for every other list, the number of entries
// that go ahead of it -- a binary search over that list's order words.  Only Key::hi (score order, inverted global video) takes part:
// the two low fields of smin_search_merge's key are (list, position), which the rank spells out as ">=" for the lists before s, ">"
// for those after, and p itself.

// The number of the n words at a (descending) that go ahead of `mine`: those >= mine (or_equal) or > mine.  n <= CORPUS_MAX_K, so
// seven halvings; every index read is < n whatever the words hold.
__device__ __forceinline__ int count_ahead(const u64* a, int n, u64 mine, bool or_equal)
{
    int lo = 0;
#pragma unroll
    for (int step = CORPUS_MAX_K; step >= 1; step >>= 1) {
        const int m = lo + step;
        if (m <= n && (or_equal ? a[m - 1] >= mine : a[m - 1] > mine)) lo = m;
    }
    return lo;
}

// One workgroup per query.  The order words of all candidates go to LDS (list s at base[s], 8 KB at most), every output slot is set
// to the empty pattern, and after one barrier each candidate whose rank is below nk moves its five fields to that slot.  For lists
// ordered as assumed the ranks are a permutation of 0 .. sum(cnt) - 1: each slot below nk is written once more, by one thread.  For
// any other input rank <= p + the other lists' counts < sum(cnt), so a write stays inside the query's K slots.
__global__ __launch_bounds__(CT)
void span_search_merge_kernel(const ListTables<SpanFields> tb, const ListOut<SpanFields> out)
{
    __shared__ u64 hi[MERGE_MAX_S * CORPUS_MAX_K];
    __shared__ int cnt[MERGE_MAX_S];
    const int t = threadIdx.x, S = tb.S;
    const long long q = blockIdx.x;
    if (t < S) cnt[t] = min(max(tb.count[t][q], 0), tb.k[t]);
    out.finish(0);                                               // all K slots empty (and count 0, which thread 0 overwrites below)
    __syncthreads();
    for (int c = t; c < tb.base[S]; c += CT) {
        int s = 0;
        while (s + 1 < S && c >= tb.base[s + 1]) ++s;
        const int p = c - tb.base[s];
        if (p >= cnt[s]) continue;                               // behind the count: never read
        const long long i = q * tb.k[s] + p;
        hi[c] = video_word(tb.score[s][i], (int)(tb.video[s][i] + tb.offset[s]));
    }
    __syncthreads();
    int total = 0;
    for (int s = 0; s < S; ++s) total += cnt[s];
    const int nk = min(total, out.K);
    for (int c = t; c < tb.base[S]; c += CT) {
        int s = 0;
        while (s + 1 < S && c >= tb.base[s + 1]) ++s;
        const int p = c - tb.base[s];
        if (p >= cnt[s]) continue;
        const u64 mine = hi[c];
        int rank = p;
        for (int o = 0; o < S; ++o)
            if (o != s) rank += count_ahead(hi + tb.base[o], cnt[o], mine, o < s);
        if (rank >= nk) continue;
        const long long i = q * tb.k[s] + p;
        const size_t r = out.at(rank);
        const long long v = tb.video[s][i] + tb.offset[s];
        const float sc = tb.score[s][i];
        out.f.move(r, tb.in[s], i);
        out.video[r] = v;
        out.score[r] = sc;
    }
    if (t == 0) out.count[q] = nk;
}

// ---- hard-negative mining (smin_mine_pairs).  Query q owns the pairs q * S .. q * S + S - 1, S = 1 + N: slot 0 its own video, slots
// 1 .. N the negatives of ranks skip .. skip + N - 1.  smin_mine_pairs' candidates: c = video over row q of the pair scores, the
// query's own video left out; key parts (slot 0, w = the video, which emit reads back as its pick).
struct ScoreRow {
    const float* row /* [V] */; int gt, skip; int* picks /* the query's S entries of video_index */;
    __device__ __forceinline__ bool read(long long c, int& slot, long long& w, float& sc, int& vid) const
    {
        if ((int)c == gt) return false;
        slot = 0; w = c;
        sc = row[c];
        vid = (int)c;
        return true;
    }
    __device__ __forceinline__ void emit(int r, int, long long w) const
    {
        if (r >= skip) picks[1 + r - skip] = (int)w;
    }
};

// One workgroup per query: the lists and the grouping by query, which is the identity.  Every candidate has a nonzero key below the
// first cursor and skip + N <= V - 1, so the rounds never run dry and all N negatives are written.
__global__ __launch_bounds__(CT)
void mine_select_kernel(const float* __restrict__ score, const int* __restrict__ gt_video, int Q, int V, int N, int skip,
                        int* __restrict__ video_index, int* __restrict__ query_index, int* __restrict__ q_ptr, int* __restrict__ q_pairs)
{
    const int q = blockIdx.x, S = 1 + N, t = threadIdx.x;
    const int gt = min(max(gt_video[q], 0), V - 1);
    const ScoreRow src{score + (size_t)q * V, gt, skip, video_index + (size_t)q * S};
    topk_rounds(src, V, skip + N);
    for (int s = t; s < S; s += CT) {
        const int p = q * S + s;
        query_index[p] = q;
        q_pairs[p] = p;
    }
    if (t == 0) {
        video_index[(size_t)q * S] = gt;
        q_ptr[q] = q * S;
        if (q == Q - 1) q_ptr[Q] = Q * S;
    }
}

// The pair of query q that names video v, or -1: a query's S picks are distinct videos, so there is at most one.
__device__ __forceinline__ int pair_of(const int* __restrict__ video_index, int q, int S, int v)
{
    int p = -1;
    for (int s = 0; s < S; ++s) if (video_index[(size_t)q * S + s] == v) p = q * S + s;
    return p;
}

// One workgroup per video: the number of pairs that name it.
__global__ __launch_bounds__(CT)
void mine_count_kernel(const int* __restrict__ video_index, int Q, int S, int* __restrict__ counts /* [V] */)
{
    __shared__ int red[CT / 64];
    const int v = blockIdx.x;
    int n = 0;
    for (int q = threadIdx.x; q < Q; q += CT) n += pair_of(video_index, q, S, v) >= 0;
    n = block_sum(n, red);
    if (threadIdx.x == 0) counts[v] = n;
}

// One workgroup: v_ptr = the exclusive prefix of the counts, CT videos at a time in ascending v (integer sums: any order gives the
// same bits; this one needs a single pass).
__global__ __launch_bounds__(CT)
void mine_scan_kernel(const int* __restrict__ counts, int V, int* __restrict__ v_ptr /* [V + 1] */)
{
    __shared__ int wave_sum[CT / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int base = 0;
    for (int v0 = 0; v0 < V; v0 += CT) {
        const int v = v0 + t;
        const int c = v < V ? counts[v] : 0;
        int incl = c;
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        __syncthreads();                                         // (the previous chunk's reads of wave_sum are done)
        if (lane == 63) wave_sum[wv] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CT / 64; ++w) {
            if (w < wv) before += wave_sum[w];
            total += wave_sum[w];
        }
        if (v < V) v_ptr[v] = base + before + incl - c;
        base += total;
    }
    if (t == 0) v_ptr[V] = base;
}

// One workgroup per video: its pairs in ascending p, which is ascending q -- CT queries at a time, each chunk's pairs placed by a
// ballot prefix within the wave and the waves' totals in order.  Plain stores, no atomics: the same bits every run.
__global__ __launch_bounds__(CT)
void mine_fill_kernel(const int* __restrict__ video_index, const int* __restrict__ v_ptr, int Q, int S, int* __restrict__ v_pairs /* [P] */)
{
    __shared__ int red[CT / 64];
    const int v = blockIdx.x, t = threadIdx.x;
    const long long P = (long long)Q * S;
    long long base = v_ptr[v];
    for (int q0 = 0; q0 < Q; q0 += CT) {
        const int q = q0 + t;
        const int p = q < Q ? pair_of(video_index, q, S, v) : -1;
        int total;
        const long long o = base + block_scan_flag(p >= 0, red, total);
        if (p >= 0 && o >= 0 && o < P) v_pairs[o] = p;
        base += total;
    }
}

// ---- merge of shard lists that carry their unweighted scores (smin_search_merge_weighted, smin_span_search_merge_weighted;
// INTEGRATION.md 3u).  A candidate's value is raw * video_weight[q][g], g its global video, and the videos the corpus-wide rank cuts
// drop out, so the lists are NOT sorted in the order they are merged in (rounding under the new weight may swap near-ties): no
// binary search.  One workgroup per query stages the order word of every candidate in LDS (0 for one that dropped out; at most
// 16 * 64 words, 8 KB) and each candidate counts the words ahead of it, as video_rank_kernel does: a larger word, or an equal one
// earlier in (list, position) order.  That order is strict and total, so the survivors' ranks are a permutation of 0 .. n - 1 and,
// after the fill with the empty pattern, each slot below nk = min(n, K) has exactly one writer.  The tables' score column holds the
// lists' raw scores; the output has a raw column beside the weighted score.
constexpr int WM_OWN = MERGE_MAX_S * CORPUS_MAX_K / CT;          // candidates a thread owns at most: c = t, t + CT, ...

template <class F>
__global__ __launch_bounds__(CT)
void merge_weighted_kernel(const ListTables<F> tb, const int* __restrict__ video_rank, const float* __restrict__ video_weight, int V,
                           int max_videos, const ListOut<F> out, float* __restrict__ out_raw /* [Q][K] */)
{
    __shared__ u64 word[MERGE_MAX_S * CORPUS_MAX_K];
    __shared__ int cnt[MERGE_MAX_S];
    __shared__ int red[CT / 64];
    const int t = threadIdx.x, S = tb.S, ncand = tb.base[S];
    const long long q = blockIdx.x;
    if (t < S) cnt[t] = min(max(tb.count[t][q], 0), tb.k[t]);
    for (int r = t; r < out.K; r += CT) {                         // all K slots empty
        const size_t o = out.at(r);
        out.clear(o);
        out_raw[o] = 0.f;
    }
    __syncthreads();
    const int nown = (ncand + CT - 1) / CT;                       // (uniform)
    u64 mine[WM_OWN];
    float val[WM_OWN];
    long long src[WM_OWN];
    int lst[WM_OWN], gvid[WM_OWN], alive = 0;
#pragma unroll
    for (int r = 0; r < WM_OWN; ++r) {
        const int c = t + r * CT;
        mine[r] = 0ull; val[r] = 0.f; src[r] = 0; lst[r] = 0; gvid[r] = 0;
        if (c >= ncand) continue;
        int s = 0;
        while (s + 1 < S && c >= tb.base[s + 1]) ++s;
        const int p = c - tb.base[s];
        if (p < cnt[s]) {                                        // behind the count: never read
            const long long i = q * tb.k[s] + p;
            const long long g = tb.video[s][i] + tb.offset[s];
            if (g >= 0 && g < V) {                               // (g forms no address before this)
                const size_t e = (size_t)q * V + (size_t)g;
                const int vr = video_rank[e];
                if (vr >= 0 && (max_videos <= 0 || vr < max_videos)) {
                    val[r] = tb.score[s][i] * video_weight[e];   // smin_moment_reweight's product
                    mine[r] = video_word(val[r], (int)g);        // >= 2^32: never the 0 of a dropped candidate
                    src[r] = i; lst[r] = s; gvid[r] = (int)g;
                    ++alive;
                }
            }
        }
        word[c] = mine[r];
    }
    const int nk = min(block_sum(alive, red), out.K);             // (its barriers also publish the stage)
    int rank[WM_OWN];
#pragma unroll
    for (int r = 0; r < WM_OWN; ++r) rank[r] = 0;
    for (int j = 0; j < ncand; ++j) {                             // one LDS address for the whole wave: a broadcast
        const u64 w = word[j];
#pragma unroll
        for (int r = 0; r < WM_OWN; ++r)
            if (r < nown) rank[r] += (w > mine[r]) || (w == mine[r] && j < t + r * CT);
    }
#pragma unroll
    for (int r = 0; r < WM_OWN; ++r) {
        if (mine[r] == 0ull || rank[r] >= nk) continue;
        const size_t o = out.at(rank[r]);
        const int s = lst[r];
        const float raw = tb.score[s][src[r]];
        out.f.move(o, tb.in[s], src[r]);
        out.video[o] = gvid[r];
        out.score[o] = val[r];
        out_raw[o] = raw;
    }
    if (t == 0) out.count[q] = nk;
}

// An output that is the input p (NULL is none): a kernel would read it while other threads write the result.
bool aliased(const void* p, const void* const* outs, int n_out)
{
    for (int o = 0; o < n_out; ++o)
        if (p != nullptr && p == outs[o]) return true;
    return false;
}

// What the four merges check and fill alike.  fields: F::N arrays of S tables, in the order F::in() reads them; outs: every output.
// With Q == 0 it returns 0 after the checks of S, K, Q and a given k_list, and the caller has nothing to launch.
template <class F>
int fill_tables(ListTables<F>& tb, int S, const int64_t* const* video, const float* const* score, const int32_t* const* count,
                const void* const* const* fields, const int32_t* k_list, const int64_t* video_offset, int Q, int K,
                const void* const* outs, int n_out)
{
    SMIN_REQUIRE(S >= 1 && S <= MERGE_MAX_S && K >= 1 && K <= CORPUS_MAX_K && Q >= 0);
    tb.S = S;
    if (k_list) {
        for (int s = 0; s < S; ++s) {
            SMIN_REQUIRE(k_list[s] >= 1 && k_list[s] <= CORPUS_MAX_K);
            tb.k[s] = k_list[s];
            tb.base[s + 1] = tb.base[s] + k_list[s];
        }
    }
    if (Q == 0) return 0;
    SMIN_REQUIRE(video != nullptr && score != nullptr && count != nullptr && k_list != nullptr && video_offset != nullptr);
    for (int c = 0; c < F::N; ++c) SMIN_REQUIRE(fields[c] != nullptr);
    for (int o = 0; o < n_out; ++o) SMIN_REQUIRE(outs[o] != nullptr);
    for (int s = 0; s < S; ++s) {
        SMIN_REQUIRE(video_offset[s] >= 0 && video_offset[s] <= 0x7fffffffll);
        const void* in[3 + F::N] = {video[s], score[s], count[s]};
        for (int c = 0; c < F::N; ++c) in[3 + c] = fields[c][s];
        for (const void* p : in) SMIN_REQUIRE(p != nullptr && !aliased(p, outs, n_out));
        tb.video[s] = (const long long*)video[s]; tb.score[s] = score[s]; tb.count[s] = count[s];
        tb.in[s] = F::in(in + 3);
        tb.offset[s] = video_offset[s];
    }
    return 0;
}

// The weighted merges': the video tables of the whole corpus beside the lists.
template <class F>
int fill_weighted_tables(ListTables<F>& tb, int S, const int64_t* const* video, const float* const* raw, const int32_t* const* count,
                         const void* const* const* fields, const int32_t* k_list, const int64_t* video_offset, const int32_t* video_rank,
                         const float* video_weight, int V, int Q, int K, const void* const* outs, int n_out)
{
    SMIN_REQUIRE(V >= 0);
    const int rc = fill_tables(tb, S, video, raw, count, fields, k_list, video_offset, Q, K, outs, n_out);
    if (rc != 0 || Q == 0) return rc;
    SMIN_REQUIRE(V == 0 || (video_rank != nullptr && video_weight != nullptr));      // (V == 0: every candidate drops out, neither is read)
    SMIN_REQUIRE(!aliased(video_rank, outs, n_out) && !aliased(video_weight, outs, n_out));
    return 0;
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
    const ListOut<IdxFields> out{(long long*)out_video, out_score, out_count, {(long long*)out_idx}, K};
    hipLaunchKernelGGL(group_topk_kernel<IdxFields>, dim3(Q), dim3(CT), 0, (hipStream_t)stream, pair_score, pair_count, pair_video, pair_ptr,
                       IdxFields::In{(const long long*)pair_idx}, k_video, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_search_merge(void* stream, int S, const int64_t* const* video, const int64_t* const* idx, const float* const* score,
                                 const int32_t* const* count, const int32_t* k_list, const int64_t* video_offset, int Q, int K,
                                 int64_t* out_video, int64_t* out_idx, float* out_score, int32_t* out_count)
{
    ListTables<IdxFields> tb{};
    const void* const* fields[1] = {(const void* const*)idx};
    const void* outs[4] = {out_video, out_idx, out_score, out_count};
    const int rc = fill_tables(tb, S, video, score, count, fields, k_list, video_offset, Q, K, outs, 4);
    if (rc != 0 || Q == 0) return rc;
    const ListOut<IdxFields> out{(long long*)out_video, out_score, out_count, {(long long*)out_idx}, K};
    hipLaunchKernelGGL(search_merge_kernel, dim3(Q), dim3(CT), 0, (hipStream_t)stream, tb, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_corpus_span_topk(void* stream, const float* span, const float* score, const int64_t* window, const int64_t* cell,
                                     const int32_t* count, const int32_t* group_video, const int32_t* group_ptr, int Q, int k_video, int K,
                                     int64_t* out_video, float* out_span, float* out_score, int64_t* out_window, int64_t* out_cell,
                                     int32_t* out_count)
{
    SMIN_REQUIRE(K >= 1 && K <= CORPUS_MAX_K && k_video >= 1 && k_video <= CORPUS_MAX_K && Q >= 0);
    if (Q == 0) return 0;
    SMIN_REQUIRE(group_ptr != nullptr && out_video != nullptr && out_span != nullptr && out_score != nullptr && out_window != nullptr);
    SMIN_REQUIRE(out_cell != nullptr && out_count != nullptr);
    // (as smin_corpus_topk: with a NULL list the kernel reads none of the six and every query comes out empty)
    const ListOut<SpanFields> out{(long long*)out_video, out_score, out_count, {out_span, (long long*)out_window, (long long*)out_cell}, K};
    hipLaunchKernelGGL(group_topk_kernel<SpanFields>, dim3(Q), dim3(CT), 0, (hipStream_t)stream, score, count, group_video, group_ptr,
                       SpanFields::In{span, (const long long*)window, (const long long*)cell}, k_video, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_span_search_merge(void* stream, int S, const int64_t* const* video, const float* const* span, const float* const* score,
                                      const int64_t* const* window, const int64_t* const* cell, const int32_t* const* count,
                                      const int32_t* k_list, const int64_t* video_offset, int Q, int K, int64_t* out_video, float* out_span,
                                      float* out_score, int64_t* out_window, int64_t* out_cell, int32_t* out_count)
{
    ListTables<SpanFields> tb{};
    const void* const* fields[3] = {(const void* const*)span, (const void* const*)window, (const void* const*)cell};
    const void* outs[6] = {out_video, out_span, out_score, out_window, out_cell, out_count};
    const int rc = fill_tables(tb, S, video, score, count, fields, k_list, video_offset, Q, K, outs, 6);
    if (rc != 0 || Q == 0) return rc;
    const ListOut<SpanFields> out{(long long*)out_video, out_score, out_count, {out_span, (long long*)out_window, (long long*)out_cell}, K};
    hipLaunchKernelGGL(span_search_merge_kernel, dim3(Q), dim3(CT), 0, (hipStream_t)stream, tb, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_search_merge_weighted(void* stream, int S, const int64_t* const* video, const int64_t* const* idx, const float* const* raw,
                                          const int32_t* const* count, const int32_t* k_list, const int64_t* video_offset,
                                          const int32_t* video_rank, const float* video_weight, int V, int max_videos, int Q, int K,
                                          int64_t* out_video, int64_t* out_idx, float* out_score, float* out_raw, int32_t* out_count)
{
    ListTables<IdxFields> tb{};
    const void* const* fields[1] = {(const void* const*)idx};
    const void* outs[5] = {out_video, out_idx, out_score, out_raw, out_count};
    const int rc = fill_weighted_tables(tb, S, video, raw, count, fields, k_list, video_offset, video_rank, video_weight, V, Q, K, outs, 5);
    if (rc != 0 || Q == 0) return rc;
    const ListOut<IdxFields> out{(long long*)out_video, out_score, out_count, {(long long*)out_idx}, K};
    hipLaunchKernelGGL(merge_weighted_kernel<IdxFields>, dim3(Q), dim3(CT), 0, (hipStream_t)stream, tb, video_rank, video_weight, V, max_videos, out,
                       out_raw);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_span_search_merge_weighted(void* stream, int S, const int64_t* const* video, const float* const* span, const float* const* raw,
                                               const int64_t* const* window, const int64_t* const* cell, const int32_t* const* count,
                                               const int32_t* k_list, const int64_t* video_offset, const int32_t* video_rank,
                                               const float* video_weight, int V, int max_videos, int Q, int K, int64_t* out_video, float* out_span,
                                               float* out_score, float* out_raw, int64_t* out_window, int64_t* out_cell, int32_t* out_count)
{
    ListTables<SpanFields> tb{};
    const void* const* fields[3] = {(const void* const*)span, (const void* const*)window, (const void* const*)cell};
    const void* outs[7] = {out_video, out_span, out_score, out_raw, out_window, out_cell, out_count};
    const int rc = fill_weighted_tables(tb, S, video, raw, count, fields, k_list, video_offset, video_rank, video_weight, V, Q, K, outs, 7);
    if (rc != 0 || Q == 0) return rc;
    const ListOut<SpanFields> out{(long long*)out_video, out_score, out_count, {out_span, (long long*)out_window, (long long*)out_cell}, K};
    hipLaunchKernelGGL(merge_weighted_kernel<SpanFields>, dim3(Q), dim3(CT), 0, (hipStream_t)stream, tb, video_rank, video_weight, V, max_videos, out,
                       out_raw);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_mine_pairs_ws_bytes(int Q, int V, int N)
{
    if (Q < 1 || V < 2 || N < 1) return 0;
    return (size_t)V * sizeof(int);                              // the videos' pair counts
}

extern "C" int smin_mine_pairs(void* stream, const float* score, const int32_t* gt_video, int Q, int V, int N, int skip, int32_t* video_index,
                               int32_t* query_index, int32_t* v_ptr, int32_t* v_pairs, int32_t* q_ptr, int32_t* q_pairs, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(Q >= 1 && V >= 2 && N >= 1 && skip >= 0 && skip <= CORPUS_MAX_K && N <= CORPUS_MAX_K);
    SMIN_REQUIRE(skip + N <= CORPUS_MAX_K && skip + N <= V - 1 && (long long)Q * (1 + N) < 0x80000000ll);
    SMIN_REQUIRE(score != nullptr && gt_video != nullptr && video_index != nullptr && query_index != nullptr);
    SMIN_REQUIRE(v_ptr != nullptr && v_pairs != nullptr && q_ptr != nullptr && q_pairs != nullptr);
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= smin_mine_pairs_ws_bytes(Q, V, N));
    const hipStream_t st = (hipStream_t)stream;
    int* counts = static_cast<int*>(ws);
    hipLaunchKernelGGL(mine_select_kernel, dim3(Q), dim3(CT), 0, st, score, gt_video, Q, V, N, skip, video_index, query_index, q_ptr, q_pairs);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mine_count_kernel, dim3(V), dim3(CT), 0, st, video_index, Q, 1 + N, counts);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mine_scan_kernel, dim3(1), dim3(CT), 0, st, counts, V, v_ptr);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mine_fill_kernel, dim3(V), dim3(CT), 0, st, video_index, v_ptr, Q, 1 + N, v_pairs);
    SMIN_LAUNCH_CHECK();
    return 0;
}
