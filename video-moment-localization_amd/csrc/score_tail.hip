// Forward-only tail of a scorer: the LAST SMI layer's moment unit (reference models.py:288-303) and the map's score head
// (models.py:337) multiplied out.  Nobody but the score head reads the last mu, so with w, beta = conv_layer_pm.{weight, bias}
//   a = Wfb^T w    c = Wfc^T w    u = Wc^T c    k0 = bc.c + w.bcat + beta
//   logit[n] = sum_d a[d] bu[b,i,d] bu[b,j,d] + ccmean[n].u + (cumean[n] + hbar[n]).c + fm[n].w + k0        pm = sigmoid(logit)
// which is exact in real arithmetic (a re-association of the same products).  Three launches besides the boundary
// heads: the vectors a, c (column sums of Wcat scaled by w), the vector u and k0 -- parameters only, a stage a host may issue early
// on another stream --, and one streaming pass over the cells.
// The streaming pass is HBM-bound: per cell it reads dl + 3D floats (dl + 2D when hbar is re-formed from fm and fs) and two rows of
// bu that stay in L2 (the list is sorted by (b, i, j): a wave's cells share row i and walk j).  All arithmetic is fp32 FMAs.
#include "common.h"
#include "smin_hip.h"

namespace smin {

constexpr int TAIL_COLS = 64;      // columns of a weight matrix per pass of a 1024-thread workgroup (x 16 row groups)
constexpr int TAIL_CPW = 8;        // consecutive cells per wave of the streaming pass (its vectors stay in registers)

// out[col] = sum_r M[r][col] * v[r] for the 64 columns from col0, rows split over 16 groups: a fixed summation order
__device__ __forceinline__ void column_dots(const float* __restrict__ M, int rows, int ld, int cols, int col0, const float* __restrict__ v,
                                            float* __restrict__ out, float (*part)[TAIL_COLS])
{
    const int lc = threadIdx.x & (TAIL_COLS - 1), g = threadIdx.x / TAIL_COLS, col = col0 + lc;
    float s = 0.f;
    if (col < cols)
        for (int r = g; r < rows; r += 16) s = fmaf(M[(size_t)r * ld + col], v[r], s);
    part[g][lc] = s;
    __syncthreads();
    if (g == 0 && col < cols) {
        float t = part[0][lc];
        for (int k = 1; k < 16; ++k) t += part[k][lc];
        out[col] = t;
    }
    __syncthreads();
}

// ac[0..D) = a, ac[D..2D) = c : the columns of Wcat [D][2D] against w
__global__ __launch_bounds__(1024)
void tail_vectors_kernel(const float* __restrict__ Wcat, const float* __restrict__ wm, int D, float* __restrict__ ac)
{
    __shared__ float part[16][TAIL_COLS];
    column_dots(Wcat, D, 2 * D, 2 * D, blockIdx.x * TAIL_COLS, wm, ac, part);
}

// u = Wc^T c (Wc [D][dl]) and k0 = bc.c + w.bcat + beta ; one workgroup
__global__ __launch_bounds__(1024)
void tail_consts_kernel(const float* __restrict__ Wc, const float* __restrict__ bc, const float* __restrict__ bcat, const float* __restrict__ wm,
                        const float* __restrict__ bm, int D, int dl, const float* __restrict__ c, float* __restrict__ u, float* __restrict__ k0)
{
    __shared__ float part[16][TAIL_COLS];
    for (int col0 = 0; col0 < dl; col0 += TAIL_COLS) column_dots(Wc, D, dl, dl, col0, c, u, part);
    if (threadIdx.x < 64) {
        float s = 0.f;
        for (int d = threadIdx.x; d < D; d += 64) { s = fmaf(bc[d], c[d], s); s = fmaf(wm[d], bcat[d], s); }
        s = wave_sum(s);
        if (threadIdx.x == 0) k0[0] = s + bm[0];
    }
}

// hbar of four features (csrc/gate.hip's arithmetic)
__device__ __forceinline__ float4 gate4(float4 x, float4 s)
{
    return make_float4(x.x / (1.0f + expf(-x.x * s.x)), x.y / (1.0f + expf(-x.y * s.y)), x.z / (1.0f + expf(-x.z * s.z)), x.w / (1.0f + expf(-x.w * s.w)));
}
// four features of a cell's logit: a * (bu_i * bu_j) + c * (cumean + hbar) + w * fm
__device__ __forceinline__ float tail_dot4(float acc, float4 a, float4 c, float4 w, float4 bi, float4 bj, float4 q, float4 h, float4 x)
{
    acc = fmaf(a.x, bi.x * bj.x, acc); acc = fmaf(c.x, q.x + h.x, acc); acc = fmaf(w.x, x.x, acc);
    acc = fmaf(a.y, bi.y * bj.y, acc); acc = fmaf(c.y, q.y + h.y, acc); acc = fmaf(w.y, x.y, acc);
    acc = fmaf(a.z, bi.z * bj.z, acc); acc = fmaf(c.z, q.z + h.z, acc); acc = fmaf(w.z, x.z, acc);
    acc = fmaf(a.w, bi.w * bj.w, acc); acc = fmaf(c.w, q.w + h.w, acc); acc = fmaf(w.w, x.w, acc);
    return acc;
}
__device__ __forceinline__ float dot4(float acc, float4 u, float4 x)
{
    acc = fmaf(u.x, x.x, acc); acc = fmaf(u.y, x.y, acc); acc = fmaf(u.z, x.z, acc); acc = fmaf(u.w, x.w, acc);
    return acc;
}

// One wave per TAIL_CPW consecutive cells, a lane per four features.  NV > 0: D <= 256 * NV and dl <= 256, the vectors a, c, w, u
// live in registers across the wave's cells; NV == 0: any D and dl, the vectors are read (from L2) per cell.
template <int NV, bool HBAR>
__global__ __launch_bounds__(256)
void score_tail_kernel(const float* __restrict__ ccmean, const float* __restrict__ cumean, const float* __restrict__ hbar, const float* __restrict__ fm,
                       const float* __restrict__ fs, const float* __restrict__ bu, const int* __restrict__ cells, int N, int L, int D, int dl,
                       const float* __restrict__ ac, const float* __restrict__ u, const float* __restrict__ k0p, const float* __restrict__ wm,
                       float* __restrict__ pm)
{
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * TAIL_CPW;
    if (n0 >= N) return;
    const int n1 = min(N, n0 + TAIL_CPW);
    const float k0 = k0p[0];
    constexpr int NR = NV > 0 ? NV : 1;
    float4 a4[NR], c4[NR], w4[NR], u4 = f4zero();
    if (NV > 0) {
#pragma unroll
        for (int v = 0; v < NR; ++v) {
            const int d = lane * 4 + v * 256;
            const bool ok = d < D;
            a4[v] = ok ? ldg4(ac + d) : f4zero(); c4[v] = ok ? ldg4(ac + D + d) : f4zero(); w4[v] = ok ? ldg4(wm + d) : f4zero();
        }
        if (lane * 4 < dl) u4 = ldg4(u + lane * 4);
    }
    for (int n = n0; n < n1; ++n) {
        const Cell cl = load_cell(cells, n);
        const float* __restrict__ bi = bu + ((size_t)cl.b * L + cl.i) * D;
        const float* __restrict__ bj = bu + ((size_t)cl.b * L + cl.j) * D;
        const float* __restrict__ sb = fs + (size_t)cl.b * D;
        const size_t row = (size_t)n * D;
        float acc = 0.f;
        if (NV > 0) {
#pragma unroll
            for (int v = 0; v < NR; ++v) {
                const int d = lane * 4 + v * 256;
                if (d < D) {
                    const float4 x = ldg4(fm + row + d);
                    const float4 h = HBAR ? ldg4(hbar + row + d) : gate4(x, ldg4(sb + d));
                    acc = tail_dot4(acc, a4[v], c4[v], w4[v], ldg4(bi + d), ldg4(bj + d), ldg4(cumean + row + d), h, x);
                }
            }
            if (lane * 4 < dl) acc = dot4(acc, u4, ldg4(ccmean + (size_t)n * dl + lane * 4));
        } else {
            for (int d = lane * 4; d < D; d += 256) {
                const float4 x = ldg4(fm + row + d);
                const float4 h = HBAR ? ldg4(hbar + row + d) : gate4(x, ldg4(sb + d));
                acc = tail_dot4(acc, ldg4(ac + d), ldg4(ac + D + d), ldg4(wm + d), ldg4(bi + d), ldg4(bj + d), ldg4(cumean + row + d), h, x);
            }
            for (int d = lane * 4; d < dl; d += 256) acc = dot4(acc, ldg4(u + d), ldg4(ccmean + (size_t)n * dl + d));
        }
        acc = wave_sum(acc);
        if (lane == 0) pm[((size_t)cl.b * L + cl.i) * L + cl.j] = (1.0f / (1.0f + expf(-(acc + k0)))) * (float)cl.m;
    }
}

template <int NV>
static int launch_tail(hipStream_t st, const float* ccmean, const float* cumean, const float* hbar, const float* fm, const float* fs, const float* bu,
                       const int32_t* cells, int N, int L, int D, int dl, const float* ac, const float* u, const float* k0, const float* wm, float* pm)
{
    const dim3 grid(cdiv(N, 4 * TAIL_CPW)), block(256);
    if (hbar)
        hipLaunchKernelGGL((score_tail_kernel<NV, true>), grid, block, 0, st, ccmean, cumean, hbar, fm, fs, bu, cells, N, L, D, dl, ac, u, k0, wm, pm);
    else
        hipLaunchKernelGGL((score_tail_kernel<NV, false>), grid, block, 0, st, ccmean, cumean, hbar, fm, fs, bu, cells, N, L, D, dl, ac, u, k0, wm, pm);
    SMIN_LAUNCH_CHECK();
    return 0;
}

}  // namespace smin

using namespace smin;

// a [D] | c [D] | u [dl] | k0 (padded to 16 bytes)
extern "C" size_t smin_score_tail_ws_bytes(int B, int L, int D, int dl)
{
    (void)B; (void)L;
    if (D <= 0 || dl <= 0) return 0;
    return sizeof(float) * ((size_t)2 * D + dl + 4);
}

// the streaming pass's form: NV of score_tail_kernel
static int tail_form(int D, int dl) { return (dl > 256 || D > 512) ? 0 : D > 256 ? 2 : 1; }

extern "C" int smin_score_tail_fwd(void* stream, const float* ccmean, const float* cumean, const float* hbar, const float* fm, const float* fs, const float* bu,
                                   const int32_t* cells, int N, int B, int L, int D, int dl, const float* Wc, const float* bc, const float* Wcat, const float* bcat,
                                   const float* wm, const float* bm, const float* wb, const float* bb, const float* lmask, float* pm, float* psea, void* ws,
                                   size_t ws_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(N >= 0 && B > 0 && L > 0 && D > 0 && dl > 0);
    SMIN_REQUIRE(D % 4 == 0);
    SMIN_REQUIRE(dl % 4 == 0);
    SMIN_REQUIRE((size_t)N <= (size_t)B * L * L);
    // two stages that share nothing but ws: the vectors (parameters only; Wc == bc == Wcat == bcat == NULL skips it: ws holds them from
    // an earlier call) and the cells (pm == psea == NULL skips it), so that a host may form the vectors early, on another stream
    const bool vectors = Wc != nullptr || bc != nullptr || Wcat != nullptr || bcat != nullptr;
    const bool scores = pm != nullptr || psea != nullptr;
    SMIN_REQUIRE(vectors || scores);
    SMIN_REQUIRE(wm != nullptr);
    SMIN_REQUIRE(!vectors || (Wc != nullptr && bc != nullptr && Wcat != nullptr && bcat != nullptr && bm != nullptr));
    SMIN_REQUIRE(!scores || (pm != nullptr && psea != nullptr && bu != nullptr && wb != nullptr && bb != nullptr && lmask != nullptr));
    SMIN_REQUIRE(!scores || N == 0 || (ccmean != nullptr && cumean != nullptr && fm != nullptr && cells != nullptr && (hbar != nullptr || fs != nullptr)));
    SMIN_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0);
    SMIN_REQUIRE(ws_bytes >= smin_score_tail_ws_bytes(B, L, D, dl));
    float* ac = reinterpret_cast<float*>(ws);
    float* u = ac + (size_t)2 * D;
    float* k0 = u + dl;
    if (vectors) {
        hipLaunchKernelGGL(tail_vectors_kernel, dim3(cdiv(2 * D, TAIL_COLS)), dim3(1024), 0, st, Wcat, wm, D, ac);
        SMIN_LAUNCH_CHECK();
        hipLaunchKernelGGL(tail_consts_kernel, dim3(1), dim3(1024), 0, st, Wc, bc, bcat, wm, bm, D, dl, ac + D, u, k0);
        SMIN_LAUNCH_CHECK();
    }
    if (!scores) return 0;
    { int rc = launch_score_heads(st, bu, B, L, D, wb, bb, lmask, psea, pm); if (rc) return rc; }
    if (N == 0) return 0;
    switch (tail_form(D, dl)) {
    case 1: return launch_tail<1>(st, ccmean, cumean, hbar, fm, fs, bu, cells, N, L, D, dl, ac, u, k0, wm, pm);
    case 2: return launch_tail<2>(st, ccmean, cumean, hbar, fm, fs, bu, cells, N, L, D, dl, ac, u, k0, wm, pm);
    default: return launch_tail<0>(st, ccmean, cumean, hbar, fm, fs, bu, cells, N, L, D, dl, ac, u, k0, wm, pm);
    }
}
