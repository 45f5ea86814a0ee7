// The corpus-wide first-stage cut over shards: search(prefilter=M)'s cut kept exactly, as a running best-M per query,
// while the shards of a corpus stream past.
//   smin_prefilter_fold    folds one shard's first-stage scores (smin_prefilter_scores') into each query's M slots: the first
//                          n_new = min(M, seen + Vs) elements of the union of the slots' videos and the shard's, in the order
//                          smin_video_rank and smin_prefilter_select give one bank of all the videos; incumbents that stay keep their
//                          slots, and copy_src names, per slot, the shard video it must receive.
//   smin_survivors_admit   copies those videos' fv rows and masks from the shard's bank into the bank of survivors;
//   smin_survivors_admit_compact  the same for a compact bank (bank_codec.hip): code rows, the rows' scales and the masks.
//   smin_prefilter_gt_rank the first-stage rank of each query's own video over the corpus' concatenated scores, O(V) per query.
// How an element finds its place: by COUNTING, as smin_video_rank does -- every element of the union (old slots and shard videos
// alike) gets one 64-bit order word, the words go through LDS 2048 at a time and an element's place is the number of words larger
// than its own.  Chosen over cutting the shard with smin_video_rank + smin_prefilter_select and merging two short lists because it is
// one launch with no workspace and no intermediate rank array, the words are distinct (the global video id is part of each), so the
// places are a permutation and no tie rule has to be restated for a merge, and smin_video_rank's count over the shard is the same
// O(Vs^2 / 256) work per workgroup that this kernel does once.
// No atomics, plain stores, every slot has one writer, every count in an order that depends on the arguments only.
#include <cstdint>

#include "common.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int FT = 256;                      // threads of a workgroup
static_assert(FT == 256, "rank_order.h's block helpers are written for four waves");
constexpr int FOLD_MAX_M = 2048;             // slots per query: their order words (16 KB) and the free-slot list (8 KB) stay in LDS
constexpr int FOLD_TILE = 2048;              // order words of the shard staged in LDS at a time (16 KB)
constexpr int FOLD_OWN = 4;                  // elements a thread places per pass over the words: one LDS read serves them all
constexpr int ADMIT_CHUNK = 2048;            // float4 of an fv row copied per workgroup (32 KB)

// The order word of a video, larger = earlier: a candidate's is smin_video_rank's (score, then the lower video); a non-candidate's
// high half is 0, below every candidate's, so the non-candidates come last in ascending video.  Distinct videos, distinct words.
__device__ __forceinline__ u64 fold_word(float score, bool cand, int video)
{
    return cand ? video_word(score, video) : (u64)video_ord(video);
}

// place[r] = the number of words of the union larger than mine[r]: the n_old old words (LDS), then the shard's, staged FOLD_TILE at a
// time.  Called by every thread of the workgroup (barriers inside).
__device__ __forceinline__ void fold_places(const u64 (&mine)[FOLD_OWN], int (&place)[FOLD_OWN], const u64* oldw, int n_old, u64* tile,
                                            const float* __restrict__ sc, const float* __restrict__ cl, int Vs, int seen)
{
#pragma unroll
    for (int r = 0; r < FOLD_OWN; ++r) place[r] = 0;
    for (int j = 0; j < n_old; ++j) {
        const u64 w = oldw[j];
#pragma unroll
        for (int r = 0; r < FOLD_OWN; ++r) place[r] += w > mine[r];
    }
    for (int t0 = 0; t0 < Vs; t0 += FOLD_TILE) {
        const int tn = min(FOLD_TILE, Vs - t0);
        __syncthreads();                                         // (the previous tile's reads are done)
        for (int j = threadIdx.x; j < tn; j += FT) tile[j] = fold_word(sc[t0 + j], cl[t0 + j] > 0.f, seen + t0 + j);
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const u64 w = tile[j];
#pragma unroll
            for (int r = 0; r < FOLD_OWN; ++r) place[r] += w > mine[r];
        }
    }
}

// One workgroup per query.
// Phase 1.  The old slots' words go to LDS (the state is read here and nowhere later).
// Phase 2.  Every old slot finds its place in the union; it stays where place < n_new, else its slot is free.
// Phase 3.  The free slots -- the evicted ones and the empty slots n_old .. n_new - 1 -- in ascending order, by a scan over the slots
//           in tiles of 256.  A slot that is not free gets copy_src -1 here; slots >= n_new are written empty.
// Phase 4.  Every shard video finds its place; the admitted ones (place < n_new), in ascending local index (a scan with a running
//           count), take the free slots in order: state and copy_src of a free slot are written by the one video that gets it.
// The words are distinct, so the places are a permutation of the union and the admitted videos are exactly as many as the free slots.
// A state that breaks the invariant (a video listed twice, ids >= seen) stays in bounds: an admitted video beyond the free slots is
// dropped, a free slot beyond the admitted videos is written empty.
__global__ __launch_bounds__(FT)
void prefilter_fold_kernel(const float* __restrict__ score, const float* __restrict__ cells, int Vs, int M, int seen, int n_old, int n_new,
                           float* slot_score, float* slot_cells, int* slot_video, int* __restrict__ copy_src)
{
    __shared__ u64 oldw[FOLD_MAX_M];
    __shared__ u64 tile[FOLD_TILE];
    __shared__ int freeslot[FOLD_MAX_M];
    __shared__ uint8_t evicted[FOLD_MAX_M];
    __shared__ int red[4];
    const int q = blockIdx.x, t = threadIdx.x;
    const float* sc = score + (size_t)q * Vs;
    const float* cl = cells + (size_t)q * Vs;
    float* ss = slot_score + (size_t)q * M;
    float* sl = slot_cells + (size_t)q * M;
    int* sv = slot_video + (size_t)q * M;
    int* cs = copy_src + (size_t)q * M;
    for (int s = t; s < n_old; s += FT) oldw[s] = fold_word(ss[s], sl[s] > 0.f, sv[s]);
    __syncthreads();

    u64 mine[FOLD_OWN];
    int place[FOLD_OWN];
    for (int own0 = 0; own0 < n_old; own0 += FT * FOLD_OWN) {    // (uniform trip count: the barriers inside are reached by all)
#pragma unroll
        for (int r = 0; r < FOLD_OWN; ++r) {
            const int s = own0 + r * FT + t;
            mine[r] = s < n_old ? oldw[s] : ~0ull;
        }
        fold_places(mine, place, oldw, n_old, tile, sc, cl, Vs, seen);
#pragma unroll
        for (int r = 0; r < FOLD_OWN; ++r) {
            const int s = own0 + r * FT + t;
            if (s < n_old) evicted[s] = place[r] >= n_new;
        }
    }
    __syncthreads();

    int nfree = 0, total;
    for (int s0 = 0; s0 < M; s0 += FT) {
        const int s = s0 + t;
        const bool fr = s < n_new && (s >= n_old || evicted[s]);
        const int pos = nfree + block_scan_flag(fr, red, total);
        nfree += total;
        if (fr) freeslot[pos] = s;
        else if (s < M) {
            cs[s] = -1;
            if (s >= n_new) { ss[s] = 0.f; sl[s] = 0.f; sv[s] = -1; }
        }
    }
    __syncthreads();

    int nadm = 0;
    for (int own0 = 0; own0 < Vs; own0 += FT * FOLD_OWN) {
        float s_[FOLD_OWN], c_[FOLD_OWN];
#pragma unroll
        for (int r = 0; r < FOLD_OWN; ++r) {
            const int v = own0 + r * FT + t;
            const bool own = v < Vs;
            s_[r] = own ? sc[v] : 0.f;
            c_[r] = own ? cl[v] : 0.f;
            mine[r] = own ? fold_word(s_[r], c_[r] > 0.f, seen + v) : ~0ull;
        }
        fold_places(mine, place, oldw, n_old, tile, sc, cl, Vs, seen);
#pragma unroll
        for (int r = 0; r < FOLD_OWN; ++r) {
            const int v = own0 + r * FT + t;
            const bool adm = v < Vs && place[r] < n_new;
            const int pos = nadm + block_scan_flag(adm, red, total);
            nadm += total;
            if (adm && pos < nfree) {
                const int s = freeslot[pos];
                ss[s] = s_[r];
                sl[s] = c_[r];
                sv[s] = seen + v;
                cs[s] = v;
            }
        }
    }
    for (int pos = nadm + t; pos < nfree; pos += FT) {           // (only a state that breaks the invariant comes here)
        const int s = freeslot[pos];
        ss[s] = 0.f; sl[s] = 0.f; sv[s] = -1; cs[s] = -1;
    }
}

// One workgroup per (survivor row, chunk of its fv row) = (blockIdx.x, blockIdx.y); the workgroup of chunk 0 also copies the masks, byte
// by byte (T + L + L L bytes: no alignment is assumed).  A row whose copy_src is -1 (or names no video of the shard) is left alone.
__global__ __launch_bounds__(FT)
void survivors_admit_kernel(const int* __restrict__ copy_src, const float* __restrict__ fv, const uint8_t* __restrict__ vmask,
                            const uint8_t* __restrict__ lmask, const uint8_t* __restrict__ mm, int Vs, int T, int L, int TD4,
                            float* __restrict__ out_fv, uint8_t* __restrict__ out_vmask, uint8_t* __restrict__ out_lmask, uint8_t* __restrict__ out_mm)
{
    const int row = blockIdx.x, chunk = blockIdx.y, t = threadIdx.x;
    const int src = copy_src[row];
    if (src < 0 || src >= Vs) return;
    const float* s = fv + (size_t)src * TD4 * 4;
    float* d = out_fv + (size_t)row * TD4 * 4;
    const int i1 = min(TD4, (chunk + 1) * ADMIT_CHUNK);
    for (int i = chunk * ADMIT_CHUNK + t; i < i1; i += FT) stg4(d + 4 * (size_t)i, ldg4(s + 4 * (size_t)i));
    if (chunk != 0) return;
    const int LL = L * L;
    for (int i = t; i < T; i += FT) out_vmask[(size_t)row * T + i] = vmask[(size_t)src * T + i];
    for (int i = t; i < L; i += FT) out_lmask[(size_t)row * L + i] = lmask[(size_t)src * L + i];
    for (int i = t; i < LL; i += FT) out_mm[(size_t)row * LL + i] = mm[(size_t)src * LL + i];
}

// survivors_admit_kernel for a compact bank: a video's code row as `nw` words of type Wd (uint4 where the row's byte count is a multiple
// of 16, else 32-bit words), its T scales (has_scale: int8 banks) and the masks with the workgroup of chunk 0.
template <class Wd>
__global__ __launch_bounds__(FT)
void survivors_admit_compact_kernel(const int* __restrict__ copy_src, const Wd* __restrict__ codes, const float* __restrict__ scale,
                                    const uint8_t* __restrict__ vmask, const uint8_t* __restrict__ lmask, const uint8_t* __restrict__ mm, int Vs,
                                    int T, int L, int nw, Wd* __restrict__ out_codes, float* __restrict__ out_scale,
                                    uint8_t* __restrict__ out_vmask, uint8_t* __restrict__ out_lmask, uint8_t* __restrict__ out_mm)
{
    const int row = blockIdx.x, chunk = blockIdx.y, t = threadIdx.x;
    const int src = copy_src[row];
    if (src < 0 || src >= Vs) return;
    const Wd* s = codes + (size_t)src * nw;
    Wd* d = out_codes + (size_t)row * nw;
    const int i1 = min(nw, (chunk + 1) * ADMIT_CHUNK);
    for (int i = chunk * ADMIT_CHUNK + t; i < i1; i += FT) d[i] = s[i];
    if (chunk != 0) return;
    const int LL = L * L;
    if (scale != nullptr)
        for (int i = t; i < T; i += FT) out_scale[(size_t)row * T + i] = scale[(size_t)src * T + i];
    for (int i = t; i < T; i += FT) out_vmask[(size_t)row * T + i] = vmask[(size_t)src * T + i];
    for (int i = t; i < L; i += FT) out_lmask[(size_t)row * L + i] = lmask[(size_t)src * L + i];
    for (int i = t; i < LL; i += FT) out_mm[(size_t)row * LL + i] = mm[(size_t)src * LL + i];
}

// One workgroup per query: the candidates whose word is larger than the own video's, counted by thread (v = t, t + 256, ...), then
// over the workgroup.
__global__ __launch_bounds__(FT)
void prefilter_gt_rank_kernel(const float* __restrict__ score, const uint8_t* __restrict__ cand, const int* __restrict__ gt_video, int V,
                              int* __restrict__ gt_rank)
{
    __shared__ int red[4];
    const int q = blockIdx.x, t = threadIdx.x;
    const float* sc = score + (size_t)q * V;
    const int gt = gt_video != nullptr ? gt_video[q] : -1;
    const bool ok = gt >= 0 && gt < V && cand[gt] != 0;          // (gt forms no address before the range check)
    int n = 0;
    if (ok) {
        const u64 mine = fold_word(sc[gt], true, gt);
        for (int v = t; v < V; v += FT) n += cand[v] != 0 && fold_word(sc[v], true, v) > mine;
    }
    n = block_sum(n, red);
    if (t == 0) gt_rank[q] = ok ? n : -1;
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" int smin_prefilter_fold(void* stream, const float* score, const float* cells, int Q, int Vs, int M, int seen, int n_old,
                                   float* slot_score, float* slot_cells, int32_t* slot_video, int32_t* copy_src)
{
    SMIN_REQUIRE(Q >= 1 && Vs >= 1 && Vs <= 0x7fff0000 && M >= 1 && M <= FOLD_MAX_M && seen >= 0);
    SMIN_REQUIRE((long long)seen + Vs <= 0x7fffffffll);          // (every global video id is an int32)
    SMIN_REQUIRE(n_old == (M < seen ? M : seen));
    SMIN_REQUIRE(score && cells && slot_score && slot_cells && slot_video && copy_src);
    const long long all = (long long)seen + Vs;
    const int n_new = all < M ? (int)all : M;
    hipLaunchKernelGGL(prefilter_fold_kernel, dim3(Q), dim3(FT), 0, (hipStream_t)stream, score, cells, Vs, M, seen, n_old, n_new, slot_score,
                       slot_cells, slot_video, copy_src);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_survivors_admit(void* stream, const int32_t* copy_src, const float* fv, const uint8_t* video_mask, const uint8_t* length_mask,
                                    const uint8_t* moment_mask, int R, int Vs, int T, int L, int D, float* out_fv, uint8_t* out_video_mask,
                                    uint8_t* out_length_mask, uint8_t* out_moment_mask)
{
    SMIN_REQUIRE(R >= 1 && Vs >= 1 && T >= 1 && L >= 1 && L <= 4096 && D >= 4 && D % 4 == 0);
    SMIN_REQUIRE((long long)T * D / 4 <= (long long)ADMIT_CHUNK * 65535);
    SMIN_REQUIRE(copy_src && fv && video_mask && length_mask && moment_mask && out_fv && out_video_mask && out_length_mask && out_moment_mask);
    SMIN_REQUIRE(((uintptr_t)fv & 15) == 0 && ((uintptr_t)out_fv & 15) == 0);
    const int TD4 = (int)((long long)T * D / 4);
    hipLaunchKernelGGL(survivors_admit_kernel, dim3(R, cdiv(TD4, ADMIT_CHUNK)), dim3(FT), 0, (hipStream_t)stream, copy_src, fv, video_mask,
                       length_mask, moment_mask, Vs, T, L, TD4, out_fv, out_video_mask, out_length_mask, out_moment_mask);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_survivors_admit_compact(void* stream, const int32_t* copy_src, const void* codes, const float* scale, int mode,
                                            const uint8_t* video_mask, const uint8_t* length_mask, const uint8_t* moment_mask, int R, int Vs, int T,
                                            int L, int D, void* out_codes, float* out_scale, uint8_t* out_video_mask, uint8_t* out_length_mask,
                                            uint8_t* out_moment_mask)
{
    SMIN_REQUIRE(R >= 1 && Vs >= 1 && T >= 1 && L >= 1 && L <= 4096 && D >= 4 && D % 4 == 0);
    SMIN_REQUIRE(bank_code_ok(codes, scale, mode, 16) && bank_code_ok(out_codes, out_scale, mode, 16));
    const long long row_bytes = (long long)T * D * (mode == SMIN_BANK_BF16 ? 2 : 1);
    SMIN_REQUIRE(row_bytes / 4 <= (long long)ADMIT_CHUNK * 65535);
    SMIN_REQUIRE(copy_src && video_mask && length_mask && moment_mask && out_video_mask && out_length_mask && out_moment_mask);
    const hipStream_t st = (hipStream_t)stream;
    if (row_bytes % 16 == 0) {
        const int nw = (int)(row_bytes / 16);
        hipLaunchKernelGGL(survivors_admit_compact_kernel<uint4>, dim3(R, cdiv(nw, ADMIT_CHUNK)), dim3(FT), 0, st, copy_src, (const uint4*)codes, scale,
                           video_mask, length_mask, moment_mask, Vs, T, L, nw, (uint4*)out_codes, out_scale, out_video_mask, out_length_mask,
                           out_moment_mask);
    } else {
        const int nw = (int)(row_bytes / 4);
        hipLaunchKernelGGL(survivors_admit_compact_kernel<uint32_t>, dim3(R, cdiv(nw, ADMIT_CHUNK)), dim3(FT), 0, st, copy_src, (const uint32_t*)codes,
                           scale, video_mask, length_mask, moment_mask, Vs, T, L, nw, (uint32_t*)out_codes, out_scale, out_video_mask,
                           out_length_mask, out_moment_mask);
    }
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_prefilter_gt_rank(void* stream, const float* score, const uint8_t* cand, const int32_t* gt_video, int Q, int V,
                                      int32_t* gt_rank)
{
    SMIN_REQUIRE(Q >= 1 && V >= 1 && V <= 0x7fff0000);
    SMIN_REQUIRE(score && cand && gt_rank);
    hipLaunchKernelGGL(prefilter_gt_rank_kernel, dim3(Q), dim3(FT), 0, (hipStream_t)stream, score, cand, gt_video, V, gt_rank);
    SMIN_LAUNCH_CHECK();
    return 0;
}
