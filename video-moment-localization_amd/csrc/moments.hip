// Top-k moment retrieval with greedy temporal NMS, and R@n, IoU=m over the kept moments.
//
// Semantics, for each sample b:
//   candidates  the cells (i, j) with moment_mask[b, i, j] != 0; masked cells are never returned.
//   score       score = (pm[b,i,j] * sqrtf(ps[b,i])) * sqrtf(pe[b,j]), fp32, in this order (the formula of metrics.hip);
//               sqrtf and the IoU division are the correctly rounded ones of hipcc's default flags (no fast-math, no __fsqrt_rn).
//   order       higher score first; ties -> lower flat index i*L + j (metrics.hip better()).  A score of -0 counts as +0.
//   IoU         of two cells in clip units (moment (i, j) spans [i, j+1), dataset.get_iou):
//                 inter = max(0, min(j1, j2) + 1 - max(i1, i2)),  union = max(j1, j2) + 1 - min(i1, i2),
//                 iou = (float)inter / (float)union  (one correctly rounded fp32 division).
//   greedy NMS  walk the candidates in order; keep one unless its IoU with an already kept cell is > nms_thresh (fp32);
//               stop after k kept or when the candidates run out.  nms_thresh >= 1: no suppression (plain top-k of the valid cells).
//   empty slots index -1 and score 0; count[b] = number kept.
//   limits      1 <= k <= 64, 1 <= B <= 65535 (launch 1 puts the sample in the grid's second dimension), L >= 1 with L*L < 2^31.
//
// Order key: a 64-bit integer, larger = earlier: the score's fp32 bits mapped to an unsigned total order in the high word, and
// 0x7fffffff - flat index in the low word.  Keys are distinct per cell and never 0 (0 marks "no cell").
//
// Launches (no host read, no inter-workgroup waiting; stage order comes from the kernel boundary):
//   1. band select, grid (P, B): sample b's cells are cut into P contiguous bands; each workgroup selects the top MB = CAND / P keys of
//      its band by a three-digit (11/11/10 bit) radix select over the streamed scores and writes them with its band's count.  A band
//      with more than MB valid cells ("full") also writes its smallest selected key.
//   2. NMS, grid (B): the keys of every band that are >= the largest smallest-key of the full bands form an exact prefix of the
//      sample's candidate order (every band holds all its keys above that floor); they are sorted in LDS (bitonic) and one wave runs
//      the greedy NMS over them in blocks of 64.  If the prefix is used up before k are kept and cells remain, the workgroup itself
//      selects the next CAND keys strictly after the last one over the whole map (the same radix select, one workgroup), sorts and
//      continues -- until k are kept or the valid cells are exhausted.  Every round consumes >= 1 candidate, so the loop is
//      bounded by the cell count; the result does not depend on CAND or MB.
//   3. (metric) per-sample hit flags for every (n, m) pair from sm at the kept cells (empty slot = IoU 0), then one thread per pair
//      sums the samples in order (no float atomics).
// Soft-NMS (a pick decays what it overlaps, and the rest is ranked again) has kernels of its own in soft_nms.hip; moment_cells.h holds
// what the two files share.  The metric stage below runs behind either selection.
#include "common.h"
#include "moment_cells.h"
#include "rank_order.h"
#include "smin_hip.h"

#include <algorithm>

namespace smin {
namespace {

constexpr int MT = MOMENT_THREADS;      // threads per workgroup (4 waves)
static_assert(MT == 256, "rank_order.h's block helpers are written for four waves");
constexpr int CAND = 4096;              // candidate keys held in LDS by the NMS workgroup
constexpr int MAX_BANDS = 32;
constexpr int MIN_BAND = 1024;          // cells per band at least
constexpr int MAX_K = MOMENT_MAX_K;
constexpr int MAX_N = 64;               // metric: up to 64 values of n ...
constexpr int MAX_M = 16;               // ... and 16 thresholds m

// order word of cell c (row i, column j) of the map, 0 if it is masked or not strictly after `cursor`
__device__ __forceinline__ uint32_t cell_ord(const Map& m, int c, int i, int j, u64 cursor)
{
    if (!m.mm[c]) return 0;
    const float v = cell_score(m, c, i, j);
    const uint32_t o = score_ord(v);
    return make_key(o, c) < cursor ? o : 0u;
}

// The bin of hist[0..nb) (nb a multiple of MT, larger bin = earlier in the order) holding the need-th element counted from the top
// (need >= 1, sum(hist) >= need).  Returns it in res[0] and the count of the bins above it in res[1].
__device__ void find_bin(const int* hist, int nb, int need, int* red, int* res)
{
    const int t = threadIdx.x, per = nb / MT, lane = t & 63, w = t >> 6;
    int s = 0;
    for (int q = 0; q < per; ++q) s += hist[t * per + q];
    int inc = s;                                                 // suffix sum within the wave (lanes >= this one)
    for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_down(inc, o); if (lane + o < 64) inc += x; }
    __syncthreads();
    if (lane == 0) red[w] = inc;
    __syncthreads();
    int above = inc - s;                                         // bins of the threads after this one
    for (int u = w + 1; u < MT / 64; ++u) above += red[u];
    if (above < need && above + s >= need) {
        for (int q = per - 1; q >= 0; --q) {
            const int h = hist[t * per + q];
            if (above + h >= need) { res[0] = t * per + q; res[1] = above; break; }
            above += h;
        }
    }
    __syncthreads();
}

struct SelectLds {
    int hist[2048];
    int red[MT / 64];
    int res[2];
    int wcnt[MT / 64];
    int pos;
    int last;
};

// Exact top-`M` keys strictly after `cursor` among the cells [lo, hi) of map m, written to out[0 .. min(M, total)) in no particular
// order.  Returns (to every thread) the number of candidate cells in the range; *kappa gets the smallest key written (if any).
__device__ int select_keys(const Map& m, int lo, int hi, u64 cursor, int M, u64* out, u64* kappa, SelectLds& s)
{
    const int t = threadIdx.x;
    for (int q = t; q < 2048; q += MT) s.hist[q] = 0;
    __syncthreads();
    int cnt = 0;
    for_cells(m, lo, hi, [&](int c, int i, int j) {
        const uint32_t o = cell_ord(m, c, i, j, cursor);
        if (o) { ++cnt; atomicAdd(&s.hist[o >> 21], 1); }
    });
    const int total = block_sum(cnt, s.red);
    uint32_t T = 0; int need = 0;                                // take ord > T, and the first `need` (index order) with ord == T
    if (total > M) {
        find_bin(s.hist, 2048, M, s.red, s.res);
        const uint32_t b1 = s.res[0]; need = M - s.res[1];
        for (int q = t; q < 2048; q += MT) s.hist[q] = 0;
        __syncthreads();
        for_cells(m, lo, hi, [&](int c, int i, int j) {
            const uint32_t o = cell_ord(m, c, i, j, cursor);
            if (o && (o >> 21) == b1) atomicAdd(&s.hist[(o >> 10) & 0x7ff], 1);
        });
        __syncthreads();
        find_bin(s.hist, 2048, need, s.red, s.res);
        const uint32_t b2 = (b1 << 11) | (uint32_t)s.res[0]; need -= s.res[1];
        for (int q = t; q < 1024; q += MT) s.hist[q] = 0;
        __syncthreads();
        for_cells(m, lo, hi, [&](int c, int i, int j) {
            const uint32_t o = cell_ord(m, c, i, j, cursor);
            if (o && (o >> 10) == b2) atomicAdd(&s.hist[o & 0x3ff], 1);
        });
        __syncthreads();
        find_bin(s.hist, 1024, need, s.red, s.res);
        T = (b2 << 10) | (uint32_t)s.res[0]; need -= s.res[1];
    }
    // gather in rounds of MT cells: ranks among ord == T follow the index order (ballot prefix + per-wave counts)
    const int lane = t & 63, w = t >> 6;
    if (t == 0) { s.pos = 0; s.last = -1; }
    __syncthreads();
    int ebase = 0;
    const int dq = MT / m.L, dr = MT % m.L;
    int c = lo + t, i = c / m.L, j = c - i * m.L;
    for (int base = lo; base < hi; base += MT) {
        const uint32_t o = c < hi ? cell_ord(m, c, i, j, cursor) : 0u;
        const bool eq = o != 0 && o == T && need > 0;
        const u64 em = __ballot(eq);
        if (lane == 0) s.wcnt[w] = __popcll(em);
        __syncthreads();
        int rank = ebase + __popcll(em & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
        for (int u = 0; u < MT / 64; ++u) { const int x = s.wcnt[u]; if (u < w) rank += x; tot += x; }
        const bool take = (o != 0 && o > T) || (eq && rank < need);
        const u64 tm = __ballot(take);
        int p0 = 0;
        if (lane == 0 && tm) p0 = atomicAdd(&s.pos, __popcll(tm));
        p0 = __shfl(p0, 0);
        if (take) out[p0 + __popcll(tm & ((1ull << lane) - 1ull))] = make_key(o, c);
        if (eq && rank == need - 1) s.last = c;                  // the last (largest-index) cell taken at ord == T
        ebase += tot;
        __syncthreads();
        c += MT; i += dq; j += dr;
        if (j >= m.L) { j -= m.L; ++i; }
    }
    if (kappa && t == 0 && total > M) *kappa = make_key(T, s.last);
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(MT)
void moments_band_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                         const uint8_t* __restrict__ mm, int L, int P, int MB,
                         u64* __restrict__ keys /* [B][P][MB] */, u64* __restrict__ kappa /* [B][P] */, int* __restrict__ cnt /* [B][P] */)
{
    __shared__ SelectLds s;
    const int p = blockIdx.x, b = blockIdx.y, n = L * L;
    const size_t o = (size_t)b * n;
    const Map m{pm + o, ps + (size_t)b * L, pe + (size_t)b * L, mm + o, L, n};
    const int band = (n + P - 1) / P, lo = min(p * band, n), hi = min(lo + band, n);
    const size_t q = (size_t)b * P + p;
    u64 kap = 0;
    const int total = select_keys(m, lo, hi, ~0ull, MB, keys + q * MB, &kap, s);
    if (threadIdx.x == 0) { cnt[q] = total; kappa[q] = total > MB ? kap : 0ull; }
}

// descending bitonic sort of a[0..np) (np a power of two) in LDS
__device__ void sort_desc(u64* a, int np)
{
    for (int size = 2; size <= np; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = threadIdx.x; x < np / 2; x += MT) {
                const int lo = 2 * x - (x & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const u64 u = a[lo], v = a[hi];
                if ((u < v) == desc) { a[lo] = v; a[hi] = u; }
            }
            __syncthreads();
        }
    }
}

struct NmsLds {
    u64 keys[CAND];
    SelectLds sel;
    int ki[MAX_K], kj[MAX_K];
    u64 kk[MAX_K];
    int nk;
    u64 floor;
    int ncand;
    int full;
};

// greedy NMS of wave 0 over the sorted a[0..nc): appends to the kept set until k are kept.  Kept cell r lives in lane r's registers
// while the wave works (s.ki/kj/kk between calls).  A block of 64 candidates is tested against the kept set in parallel; inside the
// block the survivors are resolved in lane order: the earliest is kept and suppresses the later ones it overlaps (ballot masks).
__device__ void nms_block(NmsLds& s, const u64* a, int nc, int L, int k, float thr)
{
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    int nk = s.nk;
    int ki = lane < nk ? s.ki[lane] : 0, kj = lane < nk ? s.kj[lane] : 0;
    u64 kk = lane < nk ? s.kk[lane] : 0ull;
    for (int base = 0; base < nc && nk < k; base += 64) {
        const int q = base + lane;
        const bool valid = q < nc;
        const u64 key = valid ? a[q] : 0ull;
        const int c = valid ? key_cell(key) : 0, i = c / L, j = c - i * L;
        bool sup = !valid;
        for (int r = 0; r < nk; ++r) {                           // wave-uniform trip count: readlane of the kept cells
            const int i2 = __builtin_amdgcn_readlane(ki, r), j2 = __builtin_amdgcn_readlane(kj, r);
            sup = sup || cell_iou(i, j, i2, j2) > thr;
        }
        u64 alive = __ballot(!sup);
        while (alive && nk < k) {
            const int f = __ffsll((long long)alive) - 1;         // earliest surviving candidate of the block: kept
            const int fi = __shfl(i, f), fj = __shfl(j, f);
            const u64 fk = __shfl(key, f);
            if (lane == nk) { ki = fi; kj = fj; kk = fk; }
            ++nk;
            const bool kill = lane > f && cell_iou(i, j, fi, fj) > thr;
            alive &= ~__ballot(kill);
            alive &= ~(1ull << f);
        }
    }
    if (lane < nk) { s.ki[lane] = ki; s.kj[lane] = kj; s.kk[lane] = kk; }
    if (lane == 0) s.nk = nk;
}

__global__ __launch_bounds__(MT)
void moments_nms_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe,
                        const uint8_t* __restrict__ mm, int L, int P, int MB, int k, float thr,
                        const u64* __restrict__ keys, const u64* __restrict__ kappa, const int* __restrict__ cnt,
                        long long* __restrict__ idx /* [B][k][2] */, float* __restrict__ score /* [B][k] */, int* __restrict__ count /* [B] */)
{
    __shared__ NmsLds s;
    const int b = blockIdx.x, t = threadIdx.x, n = L * L;
    const size_t o = (size_t)b * n;
    const Map m{pm + o, ps + (size_t)b * L, pe + (size_t)b * L, mm + o, L, n};
    const size_t q0 = (size_t)b * P;
    if (t == 0) {
        u64 fl = 0; int full = 0;
        for (int p = 0; p < P; ++p) if (cnt[q0 + p] > MB) { full = 1; fl = max(fl, kappa[q0 + p]); }
        s.floor = fl; s.full = full; s.ncand = 0; s.nk = 0;
    }
    __syncthreads();
    // the exact prefix: every band key >= floor
    for (int x = t; x < P * MB; x += MT) {
        const int p = x / MB, r = x - p * MB;
        if (r < min(cnt[q0 + p], MB)) {
            const u64 key = keys[(q0 + p) * MB + r];
            if (key >= s.floor) s.keys[atomicAdd(&s.ncand, 1)] = key;
        }
    }
    __syncthreads();
    int nc = s.ncand;
    bool more = s.full;                                          // cells after the prefix may remain
    for (;;) {
        int np = 1;
        while (np < nc) np <<= 1;
        for (int x = nc + t; x < np; x += MT) s.keys[x] = 0ull;
        __syncthreads();
        sort_desc(s.keys, np);
        nms_block(s, s.keys, nc, L, k, thr);
        __syncthreads();
        if (s.nk >= k || !more || nc == 0) break;
        const u64 cursor = s.keys[nc - 1];
        __syncthreads();
        const int total = select_keys(m, 0, n, cursor, CAND, s.keys, nullptr, s.sel);
        nc = min(total, CAND);
        more = total > CAND;
    }
    const int nk = s.nk;
    for (int r = t; r < k; r += MT) {
        const size_t w = (size_t)b * k + r;
        if (r < nk) {
            idx[2 * w] = s.ki[r]; idx[2 * w + 1] = s.kj[r];
            score[w] = ord_score((uint32_t)(s.kk[r] >> 32));
        } else {
            idx[2 * w] = -1; idx[2 * w + 1] = -1; score[w] = 0.f;
        }
    }
    if (t == 0) count[b] = nk;
}

struct Pairs { int n[MAX_N]; float m[MAX_M]; int nn, nm; };

__global__ __launch_bounds__(MT)
void moments_hits_kernel(const long long* __restrict__ idx, const float* __restrict__ sm, int L, int k, Pairs pr,
                         float* __restrict__ hits /* [B][nn * nm] */, float* __restrict__ top1 /* [B] or null */)
{
    __shared__ float iou[MAX_K];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int r = t; r < k; r += MT) {
        const long long i = idx[((size_t)b * k + r) * 2], j = idx[((size_t)b * k + r) * 2 + 1];
        iou[r] = i >= 0 ? sm[(size_t)b * L * L + (size_t)i * L + j] : 0.f;
    }
    __syncthreads();
    const int npairs = pr.nn * pr.nm;
    for (int q = t; q < npairs; q += MT) {
        const int a = q / pr.nm, mc = q - a * pr.nm;
        bool hit = false;
        for (int r = 0; r < pr.n[a]; ++r) hit = hit || iou[r] > pr.m[mc];
        hits[(size_t)b * npairs + q] = hit ? 1.f : 0.f;
    }
    if (t == 0 && top1) top1[b] = iou[0];                        // the epoch meter's top-1 IoU: sm at the first kept cell, 0 if none
}

__global__ void moments_hits_sum_kernel(const float* __restrict__ hits, int B, int npairs, float* __restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npairs) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += hits[(size_t)b * npairs + q];
    out[q] = s;
}

// bands per sample: enough workgroups to cover the chip at small B, bands of >= MIN_BAND cells, at most MAX_BANDS
int band_count(int B, int L)
{
    const long long n = (long long)L * L;
    long long P = (512 + B - 1) / B;
    P = std::min<long long>(P, MAX_BANDS);
    P = std::min<long long>(P, (n + MIN_BAND - 1) / MIN_BAND);
    return (int)std::max<long long>(P, 1);
}

struct WsLayout { int P, MB; size_t keys, kappa, cnt, total; };

WsLayout ws_layout(int B, int L)
{
    WsLayout w;
    w.P = band_count(B, L);
    w.MB = CAND / w.P;
    w.keys = 0;
    w.kappa = moment_align256((size_t)B * w.P * w.MB * sizeof(u64));
    w.cnt = w.kappa + moment_align256((size_t)B * w.P * sizeof(u64));
    w.total = w.cnt + moment_align256((size_t)B * w.P * sizeof(int));
    return w;
}

int launch_top(hipStream_t st, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k, float thr,
               long long* idx, float* score, int* count, char* ws)
{
    const WsLayout w = ws_layout(B, L);
    u64* keys = (u64*)(ws + w.keys);
    u64* kap = (u64*)(ws + w.kappa);
    int* cnt = (int*)(ws + w.cnt);
    hipLaunchKernelGGL(moments_band_kernel, dim3(w.P, B), dim3(MT), 0, st, pm, ps, pe, mm, L, w.P, w.MB, keys, kap, cnt);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(moments_nms_kernel, dim3(B), dim3(MT), 0, st, pm, ps, pe, mm, L, w.P, w.MB, k, thr, keys, kap, cnt, idx, score, count);
    SMIN_LAUNCH_CHECK();
    return 0;
}


// ---- cross-window merge (smin_merge_window_moments): one workgroup per pair, k rounds of "the best candidate that no kept span
// suppresses" (a block argmax of order keys strictly below the previous pick), the kept spans in LDS.  Suppression only grows
// with the kept set, so round r's pick is the r-th moment the greedy walk keeps; no sort, no atomics, any candidate count.

__device__ __forceinline__ bool span_suppressed(float st, float en, const float* kst, const float* ken, int nk, float thr)
{
    for (int r = 0; r < nk; ++r)
        if (span_iou(st, en, kst[r], ken[r]) > thr) return true;
    return false;
}

__global__ __launch_bounds__(MT)
void merge_windows_kernel(MergeIn in, const long long* __restrict__ pair_ptr, int k, float thr, MergeOut out)
{
    __shared__ float kst[MAX_K], ken[MAX_K];
    __shared__ u64 red[MT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const MergePair pr = merge_pair(in, pair_ptr, b);
    u64 cursor = ~0ull;
    int nk = 0;
    for (; nk < k; ++nk) {
        u64 best = 0;
        for (int q = t; q < pr.nslot; q += MT) {
            const MergeCand x = merge_cand(in, pr.g0, q);
            if (x.slot >= in.count[x.g]) continue;
            const u64 key = make_key(score_ord(in.score[x.c]), q);
            if (key >= cursor || key <= best) continue;
            float st, en;
            cand_span(in, x, st, en);
            if (!span_suppressed(st, en, kst, ken, nk, thr)) best = key;
        }
        best = block_max(best, red);
        if (best == 0) break;                                    // every candidate is taken or suppressed
        cursor = best;
        if (t == 0) merge_record(in, out, pr.g0, key_cell(best), (size_t)b * k + nk, 0.f, kst[nk], ken[nk]);
        __syncthreads();
    }
    merge_finish(out, b, k, nk);
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" size_t smin_top_moments_ws_bytes(int B, int L, int k)
{
    if (!moment_args_ok(B, L, k)) return 0;
    return ws_layout(B, L).total;
}

extern "C" int smin_top_moments(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, int B, int L, int k,
                                float nms_thresh, long long* idx, float* score, int* count, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(moment_args_ok(B, L, k));
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= ws_layout(B, L).total);
    return launch_top((hipStream_t)stream, pm, ps, pe, mm, B, L, k, nms_thresh, idx, score, count, (char*)ws);
}

// ---- per-sample stage of the NMS metric, shared by smin_compute_ious_nms, its soft form and the epoch meter (metrics.hip): the top-k
// launches of the rule (hard: this file's; soft: soft_nms.hip's) and the hit flags [B][nn * nm] (and, for the meter, the top-1 IoU per
// sample) in the caller's scratch.  Scratch: the selection's workspace | idx | score | count | raw_score (soft rules only) | hits.
static size_t select_ws_bytes(int method, int B, int L) { return method == 0 ? ws_layout(B, L).total : soft_top_ws_total(B, L); }

size_t smin::rule_hits_stage_bytes(int method, int B, int L, int k, int nn, int nm)
{
    if (!moment_args_ok(B, L, k) || nn < 1 || nn > MAX_N || nm < 1 || nm > MAX_M || method < 0 || method > 2) return 0;
    const size_t npairs = (size_t)nn * nm;
    const size_t top = moment_align256((size_t)B * k * 2 * sizeof(long long)) + moment_align256((size_t)B * k * sizeof(float)) +
                       moment_align256((size_t)B * sizeof(int));
    const size_t raw = method == 0 ? 0 : moment_align256((size_t)B * k * sizeof(float));
    return select_ws_bytes(method, B, L) + top + raw + moment_align256((size_t)B * npairs * sizeof(float));
}

int smin::rule_hits_stage(hipStream_t st, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm, int B, int L, int k,
                          const NmsRule& rule, const int* n_list, int nn, const float* m_list, int nm, void* ws, float** hits_out, float* top1)
{
    SMIN_REQUIRE(moment_args_ok(B, L, k) && nn >= 1 && nn <= MAX_N && nm >= 1 && nm <= MAX_M && n_list && m_list);
    SMIN_REQUIRE(rule.method == 0 || soft_rule_ok(rule));
    Pairs pr{};
    pr.nn = nn; pr.nm = nm;
    for (int a = 0; a < nn; ++a) { SMIN_REQUIRE(n_list[a] >= 1 && n_list[a] <= k); pr.n[a] = n_list[a]; }
    for (int c = 0; c < nm; ++c) pr.m[c] = m_list[c];
    char* p = (char*)ws + select_ws_bytes(rule.method, B, L);
    long long* idx = (long long*)p;   p += moment_align256((size_t)B * k * 2 * sizeof(long long));
    float* score = (float*)p;         p += moment_align256((size_t)B * k * sizeof(float));
    int* count = (int*)p;             p += moment_align256((size_t)B * sizeof(int));
    float* raw = (float*)p;           p += rule.method == 0 ? 0 : moment_align256((size_t)B * k * sizeof(float));
    float* hits = (float*)p;
    const int rc = rule.method == 0 ? launch_top(st, pm, ps, pe, mm, B, L, k, rule.thr, idx, score, count, (char*)ws)
                                    : soft_top_launch(st, pm, ps, pe, mm, B, L, k, rule, idx, score, raw, count, (char*)ws);
    if (rc) return rc;
    hipLaunchKernelGGL(moments_hits_kernel, dim3(B), dim3(MT), 0, st, idx, sm, L, k, pr, hits, top1);
    SMIN_LAUNCH_CHECK();
    *hits_out = hits;
    return 0;
}

// R@n, IoU=m over the moments a rule keeps: the stage above, then the samples summed in order
static int launch_ious(hipStream_t st, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm, int B, int L, int k,
                       const NmsRule& rule, const int* n_list, int nn, const float* m_list, int nm, float* counts, void* ws)
{
    const int npairs = nn * nm;
    float* hits = nullptr;
    const int rc = rule_hits_stage(st, pm, ps, pe, mm, sm, B, L, k, rule, n_list, nn, m_list, nm, ws, &hits, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(moments_hits_sum_kernel, dim3((npairs + 63) / 64), dim3(64), 0, st, hits, B, npairs, counts);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_compute_ious_nms_ws_bytes(int B, int L, int k, int nn, int nm)
{
    return rule_hits_stage_bytes(0, B, L, k, nn, nm);
}

extern "C" int smin_compute_ious_nms(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                     int B, int L, int k, float nms_thresh, const int* n_list, int nn, const float* m_list, int nm,
                                     float* counts, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(moment_args_ok(B, L, k) && nn >= 1 && nn <= MAX_N && nm >= 1 && nm <= MAX_M && n_list && m_list);
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= smin_compute_ious_nms_ws_bytes(B, L, k, nn, nm));
    return launch_ious((hipStream_t)stream, pm, ps, pe, mm, sm, B, L, k, NmsRule{0, nms_thresh, 0.f, 0.f}, n_list, nn, m_list, nm, counts, ws);
}

extern "C" size_t smin_compute_ious_soft_ws_bytes(int B, int L, int k, int nn, int nm)
{
    return rule_hits_stage_bytes(SMIN_NMS_LINEAR, B, L, k, nn, nm);     // both soft rules carve the same scratch
}

extern "C" int smin_compute_ious_soft(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const float* sm,
                                      int B, int L, int k, int method, float nms_thresh, float sigma, const int* n_list, int nn,
                                      const float* m_list, int nm, float* counts, void* ws, size_t ws_bytes)
{
    const NmsRule rule{method, nms_thresh, sigma, -__builtin_inff()};
    SMIN_REQUIRE(soft_rule_ok(rule));
    SMIN_REQUIRE(moment_args_ok(B, L, k) && nn >= 1 && nn <= MAX_N && nm >= 1 && nm <= MAX_M && n_list && m_list);
    SMIN_REQUIRE(pm && ps && pe && mm && sm && counts);
    SMIN_REQUIRE(ws != nullptr && ws_bytes >= smin_compute_ious_soft_ws_bytes(B, L, k, nn, nm));
    return launch_ious((hipStream_t)stream, pm, ps, pe, mm, sm, B, L, k, rule, n_list, nn, m_list, nm, counts, ws);
}

extern "C" int smin_merge_window_moments(void* stream, const int64_t* idx, const float* score, const int32_t* count, const int64_t* start,
                                         const int32_t* len, const int64_t* pair_ptr, int G, int B, int T, int L, int k_window, int k,
                                         float nms_thresh, float* span, float* out_score, int64_t* window, int64_t* cell, int32_t* out_count)
{
    const MergeIn in{(const long long*)idx, score, count, (const long long*)start, len, G, T, L, k_window};
    const MergeOut out{span, out_score, nullptr, (long long*)window, (long long*)cell, out_count};
    SMIN_REQUIRE(merge_args_ok(in, pair_ptr, B, k, out));
    if (B == 0) return 0;
    hipLaunchKernelGGL(merge_windows_kernel, dim3(B), dim3(MT), 0, (hipStream_t)stream, in, (const long long*)pair_ptr, k, nms_thresh, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}
