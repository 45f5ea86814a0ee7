// Video-level contrastive loss over a pair plan: which of a query's videos is its own.
//   cell score    f[p,i,j] = (pm[p,i,j] * sqrt(max(ps[p,i], 1e-12))) * sqrt(max(pe[p,j], 1e-12))        (top_moments' order)
//   pair score    s_p = m_p + tau * log( sum_valid exp((f - m_p) / tau) / n_p ),  m_p = max_valid f;  n_p == 0: s_p = 0
//   query loss    l_q = log sum_{S_q} exp(s / gamma) - log sum_{S_q+} exp(s / gamma), each sum shifted by its own maximum:
//                 l_q = (mx - mpos) / gamma + log sum_{S_q} exp((s - mx) / gamma) - log sum_{S_q+} exp((s - mpos) / gamma)
//   loss = mean of l_q over the queries with a positive pair;  stats = [counted, hits]
// Forward: one workgroup per pair (two sweeps over its map: maximum, then the sum), one wave64 per query over its segment in
// list order (l_q, the hit flag, each pair's coefficient dloss/ds_p without 1/Nc), one thread over the queries in ascending q.
// Backward: one workgroup per pair recomputes f and the exponentials; a row sweep writes dpm and dps, a column sweep dpe.
// Every sum has an order that depends on the arguments only; no atomics; plain stores; every output element is written.
// smin_pair_distill_fwd is the same three launches with another query kernel: the KL divergence of a query's
// softmax over its pair scores from the softmax over a teacher's scores; its coefficients go through the same backward.
#include <cmath>

#include "common.h"
#include "pair_pool.h"
#include "smin_hip.h"

namespace smin {

// pool[p] = { m_p, sum_valid exp((f - m_p) / tau) } (both 0 for a pair without a valid cell), score[p] = s_p, coef[p] = 0 (the query
// pass overwrites it for every pair a segment lists).  Thread t takes cells t, t + 256, ... of the row-major map in ascending order
// (pair_pool.h: the pooling smin_pair_pool shares).
__global__ __launch_bounds__(256)
void pair_rank_pool_kernel(const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe, const uint8_t* __restrict__ mm,
                           int L, float tau, float* __restrict__ score, float* __restrict__ pool, float* __restrict__ coef)
{
    __shared__ float red[4];
    const int p = blockIdx.x;
    const PairPool r = pair_pool_cells(pm, ps, pe, mm, p, L, tau, red);
    if (threadIdx.x == 0) {
        score[p] = r.score;
        pool[2 * (size_t)p] = r.m;
        pool[2 * (size_t)p + 1] = r.sum;
        coef[p] = 0.f;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One wave64 per query, four queries per workgroup.  Lane l takes entries l, l + 64, ... of the segment in ascending order; every
// total is wave_sum of the lanes' partials.  part[q] = { l_q, counted, hit, 0 }; coef[p] = (softmax_S(p) - [p in S+] softmax_S+(p)) / gamma,
// 0 for the pairs of a query that is not counted.
__global__ __launch_bounds__(256)
void pair_rank_query_kernel(const float* __restrict__ score, const int32_t* __restrict__ q_ptr, const int32_t* __restrict__ q_pairs,
                            const int32_t* __restrict__ positive, int P, int Q, float gamma, float* __restrict__ coef, float4* __restrict__ part)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= Q) return;                                           // (the whole wave)
    const int beg = clampi(q_ptr[q], 0, P), end = clampi(q_ptr[q + 1], beg, P);
    float mx = -INFINITY, mpos = -INFINITY, mneg = -INFINITY, npos = 0.f;
    for (int e = beg + lane; e < end; e += 64) {
        const int p = clampi(q_pairs[e], 0, P - 1);
        const float s = score[p];
        mx = fmaxf(mx, s);
        if (positive[p] != 0) { mpos = fmaxf(mpos, s); npos += 1.f; } else mneg = fmaxf(mneg, s);
    }
    mx = wave_max(mx); mpos = wave_max(mpos); mneg = wave_max(mneg);
    npos = wave_sum(npos);
    const bool counted = npos > 0.f;
    // each sum is shifted by the maximum of its own terms, so both are >= 1: a positive far below the best negative still has a
    // finite logarithm and a finite coefficient at any gamma
    float zall = 0.f, zpos = 0.f;
    if (counted)
        for (int e = beg + lane; e < end; e += 64) {
            const int p = clampi(q_pairs[e], 0, P - 1);
            const float s = score[p];
            zall += expf((s - mx) / gamma);
            if (positive[p] != 0) zpos += expf((s - mpos) / gamma);
        }
    zall = wave_sum(zall); zpos = wave_sum(zpos);
    for (int e = beg + lane; e < end; e += 64) {
        const int p = clampi(q_pairs[e], 0, P - 1);
        float c = 0.f;
        if (counted) {
            const float s = score[p];
            c = (expf((s - mx) / gamma) / zall - (positive[p] != 0 ? expf((s - mpos) / gamma) / zpos : 0.f)) / gamma;
        }
        coef[p] = c;
    }
    if (lane == 0)
        part[q] = make_float4(counted ? (mx - mpos) / gamma + (logf(zall) - logf(zpos)) : 0.f, counted ? 1.f : 0.f, counted && mpos >= mneg ? 1.f : 0.f, 0.f);
}

// ---- the listwise soft-target term: KL(teacher || student) over a query's segment, the teacher one score per pair.
// What a wave finds of ONE side of a segment, the same in every lane: mx = the maximum, z = sum exp((v - mx) / temp), first = the first
// entry in list order that holds mx, bad = the number of values that are not finite.  Both sides go through this function and through
// seg_logit, in one expression order: equal values and equal temperatures give equal bits.
struct SegSoft { float mx, z, bad; int first; };

__device__ __forceinline__ int wave_min_int(int v) {
    v = min(v, __shfl_xor(v, 1));
    v = min(v, __shfl_xor(v, 2));
    v = min(v, __shfl_xor(v, 4));
    v = min(v, __shfl_xor(v, 8));
    v = min(v, __shfl_xor(v, 16));
    v = min(v, __shfl_xor(v, 32));
    return v;
}

__device__ __forceinline__ float seg_logit(float v, float mx, float temp) { return (v - mx) / temp; }

__device__ __forceinline__ SegSoft seg_softmax(const float* __restrict__ val, const int32_t* __restrict__ q_pairs, int beg, int end, int lane, int P,
                                               float temp)
{
    SegSoft r;
    float mx = -INFINITY, bad = 0.f;
    int first = 0x7fffffff;
    for (int e = beg + lane; e < end; e += 64) {
        const float v = val[clampi(q_pairs[e], 0, P - 1)];
        if (!(fabsf(v) < INFINITY)) bad += 1.f;
        if (v > mx) { mx = v; first = e; }
    }
    r.mx = wave_max(mx);
    r.first = wave_min_int(mx == r.mx ? first : 0x7fffffff);
    r.bad = wave_sum(bad);
    float z = 0.f;
    for (int e = beg + lane; e < end; e += 64) z += expf(seg_logit(val[clampi(q_pairs[e], 0, P - 1)], r.mx, temp));
    r.z = wave_sum(z);
    return r;
}

// One wave64 per query, four queries per workgroup, pair_rank_query_kernel's layout.  A query is counted when its segment lists at
// least two pairs and every teacher value in it is finite.  part[q] = { l_q, counted, agree, 0 } with l_q = sum pT * (lT - lS) (no
// logf of a probability); coef[p] = (pS - pT) / gamma, 0 for the pairs of a query that is not counted.
__global__ __launch_bounds__(256)
void pair_distill_query_kernel(const float* __restrict__ score, const float* __restrict__ teacher, const int32_t* __restrict__ q_ptr,
                               const int32_t* __restrict__ q_pairs, int P, int Q, float gamma, float gamma_teacher, float* __restrict__ coef,
                               float4* __restrict__ part)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= Q) return;                                           // (the whole wave)
    const int beg = clampi(q_ptr[q], 0, P), end = clampi(q_ptr[q + 1], beg, P);
    const SegSoft T = seg_softmax(teacher, q_pairs, beg, end, lane, P, gamma_teacher);
    const bool counted = end - beg >= 2 && T.bad == 0.f;
    float kl = 0.f, agree = 0.f;
    if (counted) {                                                // (uniform over the wave)
        const SegSoft S = seg_softmax(score, q_pairs, beg, end, lane, P, gamma);
        const float logzs = logf(S.z), logzt = logf(T.z);
        for (int e = beg + lane; e < end; e += 64) {
            const int p = clampi(q_pairs[e], 0, P - 1);
            const float xs = seg_logit(score[p], S.mx, gamma), xt = seg_logit(teacher[p], T.mx, gamma_teacher);
            const float ps = expf(xs) / S.z, pt = expf(xt) / T.z;
            kl += pt * ((xt - logzt) - (xs - logzs));
            coef[p] = (ps - pt) / gamma;
        }
        kl = wave_sum(kl);
        agree = S.first == T.first ? 1.f : 0.f;
    } else {
        for (int e = beg + lane; e < end; e += 64) coef[clampi(q_pairs[e], 0, P - 1)] = 0.f;
    }
    if (lane == 0) part[q] = make_float4(kl, counted ? 1.f : 0.f, agree, 0.f);
}

__global__ void pair_rank_final_kernel(const float4* __restrict__ part, int Q, float* __restrict__ loss, float* __restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sum = 0.f, nc = 0.f, hits = 0.f;
    for (int q = 0; q < Q; ++q) {
        const float4 v = part[q];
        sum += v.x; nc += v.y; hits += v.z;
    }
    loss[0] = nc > 0.f ? sum / nc : 0.f;
    stats[0] = nc; stats[1] = hits;
}

// g_p = dloss * coef[p] / Nc;  df = g_p * exp((f - m_p) / tau) / sum_p on the valid cells.
//   dpm[p,i,j] = df * a_i * b_j;   dps[p,i] = (sum_j df * pm * b_j) * a_i';   dpe[p,j] = (sum_i df * pm * a_i) * b_j'
// with a = sqrt(max(ps, c)), b = sqrt(max(pe, c)) and a', b' their derivatives.  Row sweep: wave w takes rows w, w + 4, ...; lane l the
// columns l, l + 64, ... in ascending order, then wave_sum.  Column sweep: columns in chunks of 64, lane l of every wave column
// chunk + l; wave w adds rows w, w + 4, ... in ascending order, the four waves are added ((w0 + w1) + (w2 + w3)).
__global__ __launch_bounds__(256)
void pair_rank_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ stats, const float* __restrict__ coef, const float* __restrict__ pool,
                          const float* __restrict__ pm, const float* __restrict__ ps, const float* __restrict__ pe, const uint8_t* __restrict__ mm,
                          int L, float tau, float* __restrict__ dpm, float* __restrict__ dps, float* __restrict__ dpe)
{
    __shared__ float col[4][64];
    const int p = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63;
    const size_t map = (size_t)p * L * L, row = (size_t)p * L;
    const float nc = stats[0], m = pool[2 * (size_t)p], sum = pool[2 * (size_t)p + 1];
    const float g = nc > 0.f ? dloss[0] * coef[p] / nc : 0.f;
    if (g == 0.f || !(sum > 0.f)) {                               // (uniform over the workgroup) nothing flows into this pair
        for (int k = t; k < L * L; k += 256) dpm[map + k] = 0.f;
        for (int k = t; k < L; k += 256) { dps[row + k] = 0.f; dpe[row + k] = 0.f; }
        return;
    }
    const float scale = g / sum;
    for (int i = w; i < L; i += 4) {
        const float x = ps[row + i], a = rank_root(x);
        float acc = 0.f;
        for (int j = lane; j < L; j += 64) {
            const size_t o = map + (size_t)i * L + j;
            float d = 0.f;
            if (mm[o]) {
                const float b = rank_root(pe[row + j]), v = pm[o];
                const float df = scale * rank_exp(rank_cell(v, a, b), m, tau);
                d = (df * a) * b;
                acc += (df * v) * b;
            }
            dpm[o] = d;
        }
        acc = wave_sum(acc);
        if (lane == 0) dps[row + i] = acc * rank_root_grad(x, a);
    }
    for (int j0 = 0; j0 < L; j0 += 64) {
        const int j = j0 + lane;
        float acc = 0.f, y = 0.f, b = 0.f;
        if (j < L) {
            y = pe[row + j]; b = rank_root(y);
            for (int i = w; i < L; i += 4) {
                const size_t o = map + (size_t)i * L + j;
                if (mm[o]) {
                    const float a = rank_root(ps[row + i]), v = pm[o];
                    acc += ((scale * rank_exp(rank_cell(v, a, b), m, tau)) * v) * a;
                }
            }
        }
        __syncthreads();                                          // (the previous chunk's reads of col are done)
        col[w][lane] = acc;
        __syncthreads();
        if (w == 0 && j < L) dpe[row + j] = ((col[0][lane] + col[1][lane]) + (col[2][lane] + col[3][lane])) * rank_root_grad(y, b);
    }
}

}  // namespace smin

using namespace smin;

extern "C" size_t smin_pair_rank_ws_bytes(int P, int Q, int L)
{
    if (P < 1 || Q < 1 || L < 1 || L > RANK_MAX_L) return 0;
    return (size_t)Q * sizeof(float4);
}

extern "C" int smin_pair_rank_fwd(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const int32_t* q_ptr,
                                  const int32_t* q_pairs, const int32_t* positive, int P, int Q, int L, float tau, float gamma, float* loss,
                                  float* stats, float* pair_score, float* coef, float* pool, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(P >= 1 && Q >= 1 && L >= 1 && L <= RANK_MAX_L);
    SMIN_REQUIRE(pm && ps && pe && mm && q_ptr && q_pairs && positive && loss && stats && pair_score && coef && pool && ws);
    SMIN_REQUIRE(rank_temperature(tau) && rank_temperature(gamma));
    SMIN_REQUIRE(ws_bytes >= smin_pair_rank_ws_bytes(P, Q, L));
    hipStream_t st = (hipStream_t)stream;
    float4* part = (float4*)ws;
    hipLaunchKernelGGL(pair_rank_pool_kernel, dim3(P), dim3(256), 0, st, pm, ps, pe, mm, L, tau, pair_score, pool, coef);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_rank_query_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, st, pair_score, q_ptr, q_pairs, positive, P, Q, gamma, coef, part);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_rank_final_kernel, dim3(1), dim3(64), 0, st, part, Q, loss, stats);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_pair_distill_ws_bytes(int P, int Q, int L) { return smin_pair_rank_ws_bytes(P, Q, L); }

extern "C" int smin_pair_distill_fwd(void* stream, const float* pm, const float* ps, const float* pe, const uint8_t* mm, const int32_t* q_ptr,
                                     const int32_t* q_pairs, const float* teacher, int P, int Q, int L, float tau, float gamma, float gamma_teacher,
                                     float* loss, float* stats, float* pair_score, float* coef, float* pool, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(P >= 1 && Q >= 1 && L >= 1 && L <= RANK_MAX_L);
    SMIN_REQUIRE(pm && ps && pe && mm && q_ptr && q_pairs && teacher && loss && stats && pair_score && coef && pool && ws);
    SMIN_REQUIRE(rank_temperature(tau) && rank_temperature(gamma) && rank_temperature(gamma_teacher));
    SMIN_REQUIRE(ws_bytes >= smin_pair_distill_ws_bytes(P, Q, L));
    hipStream_t st = (hipStream_t)stream;
    float4* part = (float4*)ws;
    hipLaunchKernelGGL(pair_rank_pool_kernel, dim3(P), dim3(256), 0, st, pm, ps, pe, mm, L, tau, pair_score, pool, coef);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_distill_query_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, st, pair_score, teacher, q_ptr, q_pairs, P, Q, gamma, gamma_teacher,
                       coef, part);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_rank_final_kernel, dim3(1), dim3(64), 0, st, part, Q, loss, stats);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_pair_rank_bwd(void* stream, const float* dloss, const float* stats, const float* coef, const float* pool, const float* pm,
                                  const float* ps, const float* pe, const uint8_t* mm, int P, int L, float tau, float* dpm, float* dps, float* dpe)
{
    SMIN_REQUIRE(P >= 1 && L >= 1 && L <= RANK_MAX_L);
    SMIN_REQUIRE(dloss && stats && coef && pool && pm && ps && pe && mm && dpm && dps && dpe);
    SMIN_REQUIRE(rank_temperature(tau));
    hipLaunchKernelGGL(pair_rank_bwd_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, dloss, stats, coef, pool, pm, ps, pe, mm, L, tau, dpm, dps, dpe);
    SMIN_LAUNCH_CHECK();
    return 0;
}
