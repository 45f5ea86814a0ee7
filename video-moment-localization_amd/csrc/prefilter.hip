// First-stage video score from the banks alone: the model with zero SMI layers -- the score heads applied to
// ProposalGeneration's output --, which is linear in the video bank, so a query's whole row of videos is one contraction over D.
//   smin_prefilter_scores  stage 1: the operand fs (.) w_h ([3Q padded to 4][D], a small kernel) and ONE contraction on the fp32 MFMA
//                          engine (launch_gemm_nt: fv [V T][D] against the operand, in the mode of smin_set_gemm_mode), stored
//                          transposed so that a pair's T projections of a head are contiguous;
//                          stage 2: one workgroup per (q, v) stages the pair's 3 T projections in LDS, forms every cell's range sum as
//                          a running sum along its row (one wave), applies the sigmoid heads (all waves) and pools the fused scores through pair_pool.h.
//   smin_prefilter_select  each query's best M videos of smin_video_rank's ranks, ascending by video, as the pair lists of a search.
// No atomics, plain stores, every output element written, every sum in an order that depends on the arguments only.
#include <cmath>

#include "common.h"
#include "gemm.h"
#include "pair_pool.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int PT = 256;                      // threads of a workgroup (pair_pool.h's reductions are written for four waves)
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

// exclusive prefix of a 0/1 flag over the workgroup's 256 threads and its total; red: 4 ints of LDS
__device__ __forceinline__ int block_scan_flag(bool flag, int* red, int& total)
{
    const unsigned long long b = __ballot(flag);
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

extern "C" int smin_prefilter_scores(void* stream, const float* fv, const float* fs, const float* w, const float* b, const uint8_t* lmask,
                                     const uint8_t* mm, int Q, int V, int T, int L, int C, int D, float tau, float* score, float* pool,
                                     float* cells, float* pm0, float* ps0, float* pe0, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(pf_sizes_ok(Q, V, T, D) && L >= 1 && L <= PF_MAX_L && T >= L && C >= 1 && C <= 0x10000);
    SMIN_REQUIRE(rank_temperature(tau));
    SMIN_REQUIRE(fv && fs && w && b && lmask && mm && score && pool && cells && ws);
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
    const int rc = launch_gemm_nt(st, PlainMat{fv, D}, PlainMat{operand, D}, EpProjT{proj, lay.ld}, V * T, lay.N3, D);
    if (rc) return rc;
    const size_t lds = sizeof(float) * ((size_t)3 * T + (size_t)L * L + 4 * L + 4);
    hipLaunchKernelGGL(prefilter_cell_kernel, dim3(V, Q), dim3(PT), lds, st, proj, lay.ld, b, lmask, mm, V, T, L, C, tau, score, pool, cells,
                       pm0, ps0, pe0);
    SMIN_LAUNCH_CHECK();
    return 0;
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
