// First-stage video score from the banks alone: the model with zero SMI layers -- the score heads applied to
// ProposalGeneration's output --, which is linear in the video bank, so a query's whole row of videos is one contraction over D.
//   smin_prefilter_scores  stage 1: the operand fs (.) w_h ([3Q padded to 4][D], a small kernel) and ONE contraction on the fp32 MFMA
//                          engine (launch_gemm_nt: fv [V T][D] against the operand, in the mode of smin_set_gemm_mode), stored
//                          transposed so that a pair's T projections of a head are contiguous;
//                          stage 2: one workgroup per (q, v) stages the pair's 3 T projections in LDS, forms every cell's range sum as
//                          a running sum along its row (one wave), applies the sigmoid heads (all waves) and pools the fused scores through pair_pool.h.
//   smin_prefilter_scores_compact  the same over a compact bank (bank_codec.hip): stage 1's A operand is a loader that decodes, so the
//                          engine sees the decoded bank's fp32 values and the result has smin_prefilter_scores' bits on them.
//   smin_prefilter_select  each query's best M videos of smin_video_rank's ranks, ascending by video, as the pair lists of a search.
//   smin_prefilter_maps_bwd  the gradients of stage 2's maps by fv, fs and the heads (described where it begins below).
// No atomics, plain stores, every output element written, every sum in an order that depends on the arguments only.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "gemm.h"
#include "pair_pool.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int PT = 256;                      // threads of a workgroup (pair_pool.h's reductions are written for four waves)
static_assert(PT == 256, "rank_order.h's block helpers are written for four waves");
constexpr int PF_MAX_L = 64;                 // a wave owns the rows of a map: one lane per row
constexpr int PF_MAX_T = 2048;               // 3 T projections + the L x L map + 4 L words in LDS: <= 41 KB per workgroup
constexpr int PF_MAX_Q = 65535;              // blockIdx.y

// The workspace of smin_prefilter_scores as float offsets (16-byte aligned pieces: N3 % 4 == 0); smin_prefilter_ws_bytes reports `end`.
struct PfLayout { int N3; size_t ld, operand, proj, end; };
static PfLayout pf_layout(int Q, int V, int T, int D)
{
    PfLayout w;
    w.N3 = cdiv(3 * Q, 4) * 4;               // the engine's N % 4 == 0: the operand's rows are padded with zeros
    w.ld = ((size_t)V * T + 3) / 4 * 4;      // row stride of the transposed projections
    w.operand = 0;
    w.proj = w.operand + (size_t)w.N3 * D;
    w.end = w.proj + (size_t)w.N3 * w.ld;
    return w;
}
static bool pf_sizes_ok(int Q, int V, int T, int D)
{
    return Q >= 1 && Q <= PF_MAX_Q && V >= 1 && T >= 1 && T <= PF_MAX_T && D >= 4 && D % 4 == 0 && (long long)V * T <= 0x7fff0000ll &&
           (long long)V * T * (3 * Q + 3) <= (1ll << 34);        // (the contraction's tile count stays far inside an int)
}

// operand [N3][D]: row 3 q + h = fs[q] (.) w[h]; rows >= 3 Q are zero
__global__ __launch_bounds__(PT)
void prefilter_operand_kernel(const float* __restrict__ fs, const float* __restrict__ w, int Q, int D, size_t total4, float* __restrict__ operand)
{
    const size_t idx = (size_t)blockIdx.x * PT + threadIdx.x;
    if (idx >= total4) return;
    const int d4 = D / 4, n = (int)(idx / d4), c = (int)(idx % d4) * 4, q = n / 3, h = n % 3;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < Q) {
        const float4 a = ldg4(fs + (size_t)q * D + c), b = ldg4(w + (size_t)h * D + c);
        o = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
    }
    stg4(operand + (size_t)n * D + c, o);
}

// proj[col][row] = acc: a wave's 32 x ncols chunk leaves column by column, 32 consecutive rows (128 bytes) per half wave
struct EpProjT {
    float* out; size_t ld;
    __device__ __forceinline__ void chunk(const float* Ws, int row0, int col0, int ncols, int M, int N, int lane) const {
        const int r = lane & 31, row = row0 + r;
        for (int c = lane >> 5; c < ncols; c += 2) {
            const int col = col0 + c;
            if (row < M && col < N) out[(size_t)col * ld + row] = Ws[r * GEMM_LDW + c];
        }
    }
};

__device__ __forceinline__ float pf_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One workgroup per (q, v) = (blockIdx.y, blockIdx.x).  LDS: a [3][T] the pair's projections, pm [L][L], ps [L], pe [L], wlen [L] and wcs [L] the
// windows' shapes, red [4].
// Phase 1.  Threads 0 .. L - 1: the shape of a window of d + 1 clips, { frames summed c cs, clip size cs } (one division each).
// Phase 2.  Wave 0, lane i: the range sums of row i.  Its windows all begin at frame i r and their ends (i r + c cs) do not decrease
// with j, so one running sum along the row, frames in ascending order, gives every cell's sum: at most T additions per row.
// Wave 1 / 2, lane i: ps / pe of clip i, its r frames in ascending order.
// Phase 3.  All threads: the pm head on the sums, cell by cell.  Then the whole workgroup pools the map (pair_pool.h).
__global__ __launch_bounds__(PT)
void prefilter_cell_kernel(const float* __restrict__ proj, size_t ld, const float* __restrict__ bias, const uint8_t* __restrict__ lmask,
                           const uint8_t* __restrict__ mm, int V, int T, int L, int C, float tau, float* __restrict__ score,
                           float* __restrict__ pool, float* __restrict__ cells, float* __restrict__ pm0, float* __restrict__ ps0,
                           float* __restrict__ pe0)
{
    extern __shared__ __attribute__((aligned(16))) float pf_smem[];
    float* a = pf_smem;
    float* pm = a + 3 * T;
    float* ps = pm + L * L;
    float* pe = ps + L;
    int* wlen = reinterpret_cast<int*>(pe + L);                  // a window of d + 1 clips sums wlen[d] = c cs frames ...
    int* wcs = wlen + L;                                         // ... in clips of wcs[d] = cs
    float* red = reinterpret_cast<float*>(wcs + L);
    const int v = blockIdx.x, q = blockIdx.y, t = threadIdx.x, r = T / L;
    const uint8_t* vmm = mm + (size_t)v * L * L;
    for (int idx = t; idx < 3 * T; idx += PT) {
        const int h = idx / T, tt = idx - h * T;
        a[idx] = proj[(size_t)(3 * q + h) * ld + (size_t)v * T + tt];
    }
    if (t < L) {
        const int n = (t + 1) * r, cs = max(1, n / C), c = min(C, n);
        wlen[t] = c * cs;
        wcs[t] = cs;
    }
    __syncthreads();
    const int wave = t >> 6, i = t & 63;
    if (wave == 0 && i < L) {
        const int s0 = i * r;
        int pos = s0;
        float run = 0.f;
        for (int j = i; j < L; ++j) {
            const int end = s0 + wlen[j - i];
            while (pos < end) run += a[pos++];
            pm[i * L + j] = run;
        }
    } else if ((wave == 1 || wave == 2) && i < L) {
        const float* ah = a + wave * T;
        float s = 0.f;
        for (int k = 0; k < r; ++k) s += ah[i * r + k];
        const float y = lmask[(size_t)v * L + i] ? pf_sigmoid(s / (float)r + bias[wave]) : 0.f;
        (wave == 1 ? ps : pe)[i] = y;
    }
    __syncthreads();
    const float bm = bias[0];
    for (int k = t; k < L * L; k += PT) {
        const int ci = k / L, d = k - ci * L - ci;               // d < 0 under the diagonal: an empty window, sum 0, cs 1
        const float sum = d >= 0 ? pm[k] : 0.f;
        const int cs = d >= 0 ? wcs[d] : 1;
        pm[k] = vmm[k] ? pf_sigmoid((sum * (1.0f / (float)cs)) / (float)C + bm) : 0.f;   // 1 / cs in fp32, as the reference stores it
    }
    __syncthreads();
    const size_t p = (size_t)q * V + v;
    if (pm0 != nullptr) {
        for (int k = t; k < L * L; k += PT) pm0[p * L * L + k] = pm[k];
        if (t < L) { ps0[p * L + t] = ps[t]; pe0[p * L + t] = pe[t]; }
    }
    const PairPool res = pair_pool_cells(pm, ps, pe, vmm, 0, L, tau, red);
    if (t == 0) {
        score[p] = res.score;
        pool[2 * p] = res.m;
        pool[2 * p + 1] = res.sum;
        cells[p] = res.cnt;
    }
}

// One workgroup per query.  Pass 1 counts the kept candidates (0 <= rank < Ms); pass 2 walks the videos in tiles of 256, ascending,
// with two running counts -- the non-candidates so far (the first `need` of them fill the list) and the kept videos so far, which is
// the video's slot: one writer per slot, ascending by video.
__global__ __launch_bounds__(PT)
void prefilter_select_kernel(const int* __restrict__ pair_rank, int V, int Ms, int* __restrict__ sel_video, int* __restrict__ sel_query)
{
    __shared__ int red[4];
    const int q = blockIdx.x, t = threadIdx.x;
    const int* rank = pair_rank + (size_t)q * V;
    int nsel = 0, total;
    for (int v0 = 0; v0 < V; v0 += PT) {
        const int v = v0 + t;
        const int rk = v < V ? rank[v] : Ms;
        block_scan_flag(rk >= 0 && rk < Ms, red, total);
        nsel += total;
    }
    const int need = Ms - nsel;
    int non_before = 0, kept_before = 0;
    for (int v0 = 0; v0 < V; v0 += PT) {
        const int v = v0 + t;
        const int rk = v < V ? rank[v] : Ms;
        const bool non = rk < 0;
        const int non_at = non_before + block_scan_flag(non, red, total);
        non_before += total;
        const bool keep = (rk >= 0 && rk < Ms) || (non && non_at < need);
        const int slot = kept_before + block_scan_flag(keep, red, total);
        kept_before += total;
        if (keep && slot < Ms) sel_video[(size_t)q * Ms + slot] = v;
    }
    for (int s = t; s < Ms; s += PT) {
        if (s >= kept_before) sel_video[(size_t)q * Ms + s] = -1;      // (ranks that are no permutation: smin_hip.h)
        sel_query[(size_t)q * Ms + s] = q;
    }
}

}  // namespace
}  // namespace smin

using namespace smin;

extern "C" size_t smin_prefilter_ws_bytes(int Q, int V, int T, int D)
{
    if (!pf_sizes_ok(Q, V, T, D)) return 0;
    return pf_layout(Q, V, T, D).end * sizeof(float);
}

// smin_prefilter_scores' body over any A operand that hands the engine the bank's fp32 values: PlainMat (fp32), PlainMatH (bf16
// codes) or CodeMatQ (int8 codes and the rows' scales).  `bank_ok`: the caller's check of the bank's pointers.
namespace smin {
namespace {
template <class AM>
int prefilter_scores_over(void* stream, const AM& bank, bool bank_ok, const float* fs, const float* w, const float* b, const uint8_t* lmask,
                          const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float tau, float* score, float* pool, float* cells,
                          float* pm0, float* ps0, float* pe0, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(pf_sizes_ok(Q, V, T, D) && L >= 1 && L <= PF_MAX_L && T >= L && C >= 1 && C <= 0x10000);
    SMIN_REQUIRE(rank_temperature(tau));
    SMIN_REQUIRE(bank_ok && fs && w && b && lmask && mm && score && pool && cells && ws);
    SMIN_REQUIRE((pm0 && ps0 && pe0) || (!pm0 && !ps0 && !pe0));
    SMIN_REQUIRE(ws_bytes >= smin_prefilter_ws_bytes(Q, V, T, D));
    const hipStream_t st = (hipStream_t)stream;
    const PfLayout lay = pf_layout(Q, V, T, D);
    float* base = static_cast<float*>(ws);
    float* operand = base + lay.operand;
    float* proj = base + lay.proj;
    const size_t total4 = (size_t)lay.N3 * (D / 4);
    hipLaunchKernelGGL(prefilter_operand_kernel, dim3((unsigned)((total4 + PT - 1) / PT)), dim3(PT), 0, st, fs, w, Q, D, total4, operand);
    SMIN_LAUNCH_CHECK();
    const int rc = launch_gemm_nt(st, bank, PlainMat{operand, D}, EpProjT{proj, lay.ld}, V * T, lay.N3, D);
    if (rc) return rc;
    const size_t lds = sizeof(float) * ((size_t)3 * T + (size_t)L * L + 4 * L + 4);
    hipLaunchKernelGGL(prefilter_cell_kernel, dim3(V, Q), dim3(PT), lds, st, proj, lay.ld, b, lmask, mm, V, T, L, C, tau, score, pool, cells,
                       pm0, ps0, pe0);
    SMIN_LAUNCH_CHECK();
    return 0;
}
}  // namespace
}  // namespace smin

extern "C" int smin_prefilter_scores(void* stream, const float* fv, const float* fs, const float* w, const float* b, const uint8_t* lmask,
                                     const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float tau, float* score, float* pool,
                                     float* cells, float* pm0, float* ps0, float* pe0, void* ws, size_t ws_bytes)
{
    return prefilter_scores_over(stream, PlainMat{fv, D}, fv != nullptr, fs, w, b, lmask, mm, Q, V, T, L, C, D, tau, score, pool, cells, pm0, ps0,
                                 pe0, ws, ws_bytes);
}

extern "C" int smin_prefilter_scores_compact(void* stream, const void* codes, const float* scale, int mode, const float* fs, const float* w,
                                             const float* b, const uint8_t* lmask, const uint8_t* mm, int Q, int V, int T, int L, int C, int D,
                                             float tau, float* score, float* pool, float* cells, float* pm0, float* ps0, float* pe0, void* ws,
                                             size_t ws_bytes)
{
    const bool ok = bank_code_ok(codes, scale, mode, bank_quad_bytes(mode));
    if (mode == SMIN_BANK_BF16)
        return prefilter_scores_over(stream, PlainMatH{static_cast<const unsigned short*>(codes), D}, ok, fs, w, b, lmask, mm, Q, V, T, L, C, D, tau,
                                     score, pool, cells, pm0, ps0, pe0, ws, ws_bytes);
    return prefilter_scores_over(stream, CodeMatQ{static_cast<const signed char*>(codes), scale, D}, ok, fs, w, b, lmask, mm, Q, V, T, L, C, D, tau,
                                 score, pool, cells, pm0, ps0, pe0, ws, ws_bytes);
}

extern "C" int smin_prefilter_select(void* stream, const int32_t* pair_rank, int Q, int V, int M, int32_t* sel_video, int32_t* sel_query)
{
    SMIN_REQUIRE(Q >= 1 && V >= 1 && V <= 0x7fff0000 && M >= 1);
    SMIN_REQUIRE(pair_rank && sel_video && sel_query);
    const int Ms = M < V ? M : V;
    hipLaunchKernelGGL(prefilter_select_kernel, dim3(Q), dim3(PT), 0, (hipStream_t)stream, pair_rank, V, Ms, sel_video, sel_query);
    SMIN_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- backward of the first-stage maps
//   smin_prefilter_maps_bwd  from gradients on (pm0, ps0, pe0) to gradients on fv, fs and the heads:
//     1. the operand transposed, opT [D][N3] (column 3 q + h = fs[q] (.) w[h], the padding columns zero: a small kernel);
//     2. one workgroup of 256 per (q, v): the heads' sigmoid slopes from the stored outputs, the pair's three partial sums of db, a
//        suffix sum of dS along every row of the map and the pair's 3 T values of da [V T][N3] (column 3 q + h);
//     3. db: the pairs' partial sums (fp64: the heads' slopes of a contrastive loss cancel over a query's videos) added over p ascending
//        and rounded once (a small kernel);
//     4. dfv = da opT^T (launch_gemm_nt, K = N3) and dop = da^T fv (launch_gemm_tn over the V T rows, slabs reduced in split order),
//        both in the mode of smin_set_gemm_mode;
//     5. dfs[q] = sum_h dop[3 q + h] (.) w[h], dw[h] = sum_q dop[3 q + h] (.) fs[q], q ascending (a small kernel).
namespace smin {
namespace {

// The workspace of smin_prefilter_maps_bwd as float offsets (every piece a multiple of 4 floats); smin_prefilter_bwd_ws_bytes reports `end`.
struct PfBwdLayout { int N3, sp; size_t da, opT, slab, dop, dbpart, end; };
static PfBwdLayout pfb_layout(int Q, int V, int T, int D)
{
    PfBwdLayout w;
    w.N3 = cdiv(3 * Q, 4) * 4;
    // row splits of the TN contraction: enough workgroups for the chip, at least 64 rows each (the arguments alone decide)
    w.sp = std::max(1, std::min(cdiv(GEMM_SLOTS, cdiv(w.N3, 128) * cdiv(D, 128)), cdiv(V * T, 64)));
    w.da = 0;                                                    // [V T][N3]
    w.opT = w.da + (size_t)V * T * w.N3;                         // [D][N3]
    w.slab = w.opT + (size_t)D * w.N3;                           // [sp][N3][D]
    w.dop = w.slab + (size_t)w.sp * w.N3 * D;                    // [N3][D]
    w.dbpart = w.dop + (size_t)w.N3 * D;                         // [Q V][4] fp64
    w.end = w.dbpart + (size_t)Q * V * 8;
    return w;
}
static bool pfb_sizes_ok(int Q, int V, int T, int D)
{
    return pf_sizes_ok(Q, V, T, D) && (long long)(3 * Q + 3) * D <= (1ll << 28);     // (the slab reduction counts dop's elements in an int)
}

// butterfly sum over the wave's 64 lanes in fp64 (a fixed order per lane)
__device__ __forceinline__ double wave_sum_f64(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// opT [D][N3]: column 3 q + h of row d = fs[q][d] * w[h][d] (the forward's operand, transposed); columns >= 3 Q are zero
__global__ __launch_bounds__(PT)
void prefilter_operand_t_kernel(const float* __restrict__ fs, const float* __restrict__ w, int Q, int D, int N3, size_t total, float* __restrict__ opT)
{
    const size_t idx = (size_t)blockIdx.x * PT + threadIdx.x;
    if (idx >= total) return;
    const int d = (int)(idx / N3), n = (int)(idx % N3), q = n / 3, h = n % 3;
    opT[idx] = q < Q ? fs[(size_t)q * D + d] * w[(size_t)h * D + d] : 0.f;
}

// One workgroup per (q, v) = (blockIdx.y, blockIdx.x).  LDS: red [12] fp64, S [L][L | 1] (dS, then its suffix sums along the rows), gs [L],
// ge [L], inv [L] (1 / cs of a window of d + 1 clips), wlen [L], first [T] (the first d whose wlen[d] exceeds a frame's offset from its
// row's start; L if none): 4 (L (L | 1) + 4 L + T + 24) bytes.
// Phase 1.  All threads: first[] by bisection of the non-decreasing wlen[]; the slopes of the three heads from the stored outputs, dS
// cell by cell, the thread's partial sums of db in fp64; the partial sums meet in wave order.
// Phase 2.  Thread t owns quarter t & 3 of row t >> 2: the quarter's suffix sums, then the later quarters' totals on top.
// Phase 3.  All threads, one frame each: the rows i = 0 .. t / r in ascending order, one lookup each -- the cells of row i that hold
// frame t are those with j - i >= first[t - i r], whose dS the suffix sum holds at that column.
__global__ __launch_bounds__(PT)
void prefilter_cell_bwd_kernel(const float* __restrict__ dpm0, const float* __restrict__ dps0, const float* __restrict__ dpe0,
                               const float* __restrict__ pm0, const float* __restrict__ ps0, const float* __restrict__ pe0,
                               const uint8_t* __restrict__ lmask, const uint8_t* __restrict__ mm, int Q, int V, int T, int L, int C, int N3,
                               float* __restrict__ da, double* __restrict__ dbpart)
{
    extern __shared__ __attribute__((aligned(16))) float pfb_smem[];
    const int LS = L | 1;
    double* red = reinterpret_cast<double*>(pfb_smem);
    float* S = pfb_smem + 24;
    float* gs = S + L * LS;
    float* ge = gs + L;
    float* inv = ge + L;
    int* wlen = reinterpret_cast<int*>(inv + L);
    int* first = wlen + L;
    const int v = blockIdx.x, q = blockIdx.y, t = threadIdx.x, r = T / L;
    const size_t p = (size_t)q * V + v;
    const uint8_t* vmm = mm + (size_t)v * L * L;
    if (t < L) {
        const int n = (t + 1) * r, cs = max(1, n / C), c = min(C, n);
        wlen[t] = c * cs;
        inv[t] = 1.0f / (float)cs;
    }
    __syncthreads();
    for (int o = t; o < T; o += PT) {
        int lo = 0, hi = L;                                      // the first d in [0, L] with wlen[d] > o
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (wlen[mid] > o) hi = mid; else lo = mid + 1;
        }
        first[o] = lo;
    }
    double accm = 0.0, accs = 0.0, acce = 0.0;
    for (int k = t; k < L * L; k += PT) {
        const int i = k / L, j = k - i * L, d = j - i;
        const float y = pm0[p * L * L + k];
        const float g = vmm[k] ? dpm0[p * L * L + k] * y * (1.0f - y) : 0.f;
        accm += (double)g;                                       // (a valid cell under the diagonal holds sigmoid(b[0]): it reaches db alone)
        S[i * LS + j] = d >= 0 ? (g * inv[d]) / (float)C : 0.f;
    }
    if (t < L) {
        const float ys = ps0[p * L + t], ye = pe0[p * L + t];
        const bool ok = lmask[(size_t)v * L + t] != 0;
        const float s = ok ? dps0[p * L + t] * ys * (1.0f - ys) : 0.f;
        const float e = ok ? dpe0[p * L + t] * ye * (1.0f - ye) : 0.f;
        gs[t] = s;
        ge[t] = e;
        accs = (double)s;
        acce = (double)e;
    }
    accm = wave_sum_f64(accm);
    accs = wave_sum_f64(accs);
    acce = wave_sum_f64(acce);
    if ((t & 63) == 0) { red[3 * (t >> 6)] = accm; red[3 * (t >> 6) + 1] = accs; red[3 * (t >> 6) + 2] = acce; }
    __syncthreads();
    if (t < 3) dbpart[4 * p + t] = ((red[t] + red[3 + t]) + red[6 + t]) + red[9 + t];
    if (t == 3) dbpart[4 * p + 3] = 0.0;

    const int row = t >> 2, seg = t & 3, Lq = (L + 3) / 4, c0 = seg * Lq, c1 = min(L, c0 + Lq);
    const bool owner = row < L && c0 < c1;
    if (owner) {
        float run = 0.f;
        for (int j = c1 - 1; j >= c0; --j) { run += S[row * LS + j]; S[row * LS + j] = run; }
    }
    __syncthreads();
    float later = 0.f;
    if (owner)
        for (int s = 3; s > seg; --s)
            if (s * Lq < L) later += S[row * LS + s * Lq];
    __syncthreads();
    if (owner)
        for (int j = c0; j < c1; ++j) S[row * LS + j] += later;
    __syncthreads();

    const int Tr = L * r, pad = N3 - 3 * Q;
    for (int tt = t; tt < T; tt += PT) {
        float am = 0.f, as = 0.f, ae = 0.f;
        if (tt < Tr) {                                           // the frames past L r reach no clip: exactly 0
            const int ci = tt / r;
            for (int i = 0; i <= ci; ++i) {
                const int col = i + first[tt - i * r];
                if (col < L) am += S[i * LS + col];
            }
            as = gs[ci] / (float)r;
            ae = ge[ci] / (float)r;
        }
        float* o = da + ((size_t)v * T + tt) * N3 + 3 * q;
        o[0] = am; o[1] = as; o[2] = ae;
        if (q == Q - 1)
            for (int k = 0; k < pad; ++k) o[3 + k] = 0.f;        // the contraction's padding columns
    }
}

// db[h] = the pairs' partial sums in fp64, p ascending within a lane's stride of 64, then the 64 lanes ascending, rounded once
__global__ __launch_bounds__(192)
void prefilter_db_kernel(const double* __restrict__ dbpart, size_t P, float* __restrict__ db)
{
    __shared__ double part[3][64];
    const int h = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (size_t p = lane; p < P; p += 64) s += dbpart[4 * p + h];
    part[h][lane] = s;
    __syncthreads();
    if (lane == 0) {
        double v = part[h][0];
        for (int k = 1; k < 64; ++k) v += part[h][k];
        db[h] = (float)v;
    }
}

// dfs [Q][D] and dw [3][D] of dop [N3][D]: elements [0, Q D) are dfs, the next 3 D are dw (q ascending)
__global__ __launch_bounds__(PT)
void prefilter_operand_bwd_kernel(const float* __restrict__ dop, const float* __restrict__ fs, const float* __restrict__ w, int Q, int D,
                                  float* __restrict__ dfs, float* __restrict__ dw)
{
    const size_t idx = (size_t)blockIdx.x * PT + threadIdx.x, nq = (size_t)Q * D;
    if (idx < nq) {
        const size_t q = idx / D, d = idx % D;
        float s = dop[(3 * q) * D + d] * w[d];
        s += dop[(3 * q + 1) * D + d] * w[(size_t)D + d];
        s += dop[(3 * q + 2) * D + d] * w[2 * (size_t)D + d];
        dfs[idx] = s;
    } else if (idx < nq + 3 * (size_t)D) {
        const size_t h = (idx - nq) / D, d = (idx - nq) % D;
        float s = 0.f;
        for (size_t q = 0; q < (size_t)Q; ++q) s += dop[(3 * q + h) * D + d] * fs[q * D + d];
        dw[idx - nq] = s;
    }
}

}  // namespace
}  // namespace smin

extern "C" size_t smin_prefilter_bwd_ws_bytes(int Q, int V, int T, int D)
{
    if (!pfb_sizes_ok(Q, V, T, D)) return 0;
    return pfb_layout(Q, V, T, D).end * sizeof(float);
}

extern "C" int smin_prefilter_maps_bwd(void* stream, const float* dpm0, const float* dps0, const float* dpe0, const float* pm0, const float* ps0,
                                       const float* pe0, const float* fv, const float* fs, const float* w, const uint8_t* lmask,
                                       const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float* dfv, float* dfs, float* dw, float* db,
                                       void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(pfb_sizes_ok(Q, V, T, D) && L >= 1 && L <= PF_MAX_L && T >= L && C >= 1 && C <= 0x10000);
    SMIN_REQUIRE(dpm0 && dps0 && dpe0 && pm0 && ps0 && pe0 && fv && fs && w && lmask && mm && dfv && dfs && dw && db && ws);
    SMIN_REQUIRE(ws_bytes >= smin_prefilter_bwd_ws_bytes(Q, V, T, D));
    SMIN_REQUIRE(((uintptr_t)ws & 15) == 0);                     // (the contractions read da in 16-byte pieces)
    const void* ins[11] = {dpm0, dps0, dpe0, pm0, ps0, pe0, fv, fs, w, lmask, mm};
    const void* outs[5] = {dfv, dfs, dw, db, ws};
    for (int o = 0; o < 5; ++o) {                                // an output that is an input or another output
        for (const void* in : ins) SMIN_REQUIRE(in != outs[o]);
        for (int k = 0; k < o; ++k) SMIN_REQUIRE(outs[k] != outs[o]);
    }
    const hipStream_t st = (hipStream_t)stream;
    const PfBwdLayout lay = pfb_layout(Q, V, T, D);
    float* base = static_cast<float*>(ws);
    float* da = base + lay.da;
    float* opT = base + lay.opT;
    float* slab = base + lay.slab;
    float* dop = base + lay.dop;
    double* dbpart = reinterpret_cast<double*>(base + lay.dbpart);
    const size_t total = (size_t)D * lay.N3;
    hipLaunchKernelGGL(prefilter_operand_t_kernel, dim3((unsigned)((total + PT - 1) / PT)), dim3(PT), 0, st, fs, w, Q, D, lay.N3, total, opT);
    SMIN_LAUNCH_CHECK();
    const size_t lds = sizeof(float) * ((size_t)L * (L | 1) + 4 * (size_t)L + T + 24);
    hipLaunchKernelGGL(prefilter_cell_bwd_kernel, dim3(V, Q), dim3(PT), lds, st, dpm0, dps0, dpe0, pm0, ps0, pe0, lmask, mm, Q, V, T, L, C, lay.N3,
                       da, dbpart);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(prefilter_db_kernel, dim3(1), dim3(192), 0, st, dbpart, (size_t)Q * V, db);
    SMIN_LAUNCH_CHECK();
    int rc = launch_gemm_nt(st, PlainMat{da, lay.N3}, PlainMat{opT, lay.N3}, EpSlabStore{dfv}, V * T, D, lay.N3);
    if (rc) return rc;
    rc = launch_gemm_tn(st, PlainMat{da, lay.N3}, PlainMat{fv, D}, slab, (float*)nullptr, V * T, lay.N3, D, lay.sp);
    if (rc) return rc;
    rc = launch_reduce_slabs(st, slab, dop, lay.N3 * D, lay.sp);
    if (rc) return rc;
    const size_t nel = ((size_t)Q + 3) * D;
    hipLaunchKernelGGL(prefilter_operand_bwd_kernel, dim3((unsigned)((nel + PT - 1) / PT)), dim3(PT), 0, st, dop, fs, w, Q, D, dfs, dw);
    SMIN_LAUNCH_CHECK();
    return 0;
}
