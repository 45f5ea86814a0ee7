// Adam / AdamW update of a whole parameter list, with the gradients' global norm, the clip coefficient and a non-finite guard formed
// on the device (smin_adam_step / smin_grad_norm, include/smin_hip.h).
//
//   update   one launch per ADAM_CAP tensors: the tensors' pointers, element counts and moment offsets travel BY VALUE in the kernel
//            arguments (AdamTable, < 4 KB), a workgroup owns one ADAM_CHUNK-element chunk of one tensor and finds the tensor in the
//            table's prefix of chunk counts.  It reads the optimizer state and never writes it.
//   close    one wave behind the update(s): step count, running powers of the betas, skipped-step counter (the update's workgroups
//            cannot advance what they all read; the closing wave of metrics.hip's meter is the same pattern).
//   norm     only with clipping or the guard: per-chunk partial sums of (double)g * (double)g (that product is exact) in a fixed
//            association, then a one-workgroup finalize that adds the partials in a fixed order.  No atomics: the same bits every run,
//            whichever of the two load paths a tensor's alignment selects.
// Every fp32 operation of the update is rounded on its own (contract off); sqrtf and / are hipcc's correctly rounded defaults.
#include "common.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {

constexpr int ADAM_CAP = 96;            // tensors per launch (the 87 of the reference configurations: one launch)
constexpr int ADAM_CHUNK = 4096;        // elements per workgroup: 16 KB, so a chunk keeps its tensor's 16-byte alignment
constexpr int ADAM_THREADS = 256;
static_assert(ADAM_THREADS == 256, "rank_order.h's block helpers are written for four waves");

struct AdamTable {
    float* p[ADAM_CAP];
    const float* g[ADAM_CAP];
    long long moff[ADAM_CAP];           // first element of the tensor's segment in exp_avg / exp_avg_sq
    long long n[ADAM_CAP];              // elements (> 0: empty tensors never enter the table)
    int cstart[ADAM_CAP + 1];           // cstart[k] = chunks of the tensors before k; cstart[nt] = the launch's workgroups
    int nt;
};
struct AdamHyper {
    double beta1, beta2, wd;
    float b1f, omb1f, b2f, omb2f, epsf, wdf;
    int wd_mode;                        // 0: none, 1: L2 term in the gradient (Adam), 2: decoupled (AdamW)
    int use_norm;                       // the norm ran for this step: state[5] is its coefficient, state[7] its flag
    int skip;                           // write nothing when state[7] is set
};
static_assert(sizeof(AdamTable) + sizeof(AdamHyper) + 64 <= 4096, "the kernel arguments must stay under 4 KB");

// the table entry whose chunks contain workgroup `bid`: the largest k with cstart[k] <= bid (every entry has at least one chunk)
__device__ __forceinline__ int table_find(const AdamTable& tb, int bid)
{
    int lo = 0, hi = tb.nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.cstart[mid] <= bid) lo = mid; else hi = mid;
    }
    return lo;
}

struct AdamScalars { float step_size, sbc2, c, lrwdf; };

__device__ __forceinline__ void adam_element(float& p, float gr, float& m, float& v, const AdamHyper& h, const AdamScalars& s)
{
#pragma clang fp contract(off)
    float g = h.use_norm ? gr * s.c : gr;
    if (h.wd_mode == 1) g = g + h.wdf * p;
    if (h.wd_mode == 2) p = p - s.lrwdf * p;
    m = h.b1f * m + h.omb1f * g;
    v = h.b2f * v + (h.omb2f * g) * g;
    p = p - s.step_size * (m / (sqrtf(v) / s.sbc2 + h.epsf));
}

__global__ __launch_bounds__(ADAM_THREADS)
void adam_update_kernel(const AdamTable tb, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, const double* __restrict__ state,
                        const AdamHyper h)
{
#pragma clang fp contract(off)
    if (h.skip && state[7] != 0.0) return;                       // a non-finite gradient: p, m and v keep their bits
    const int bid = blockIdx.x, k = table_find(tb, bid);
    const long long base = (long long)(bid - tb.cstart[k]) * ADAM_CHUNK;
    const long long left = tb.n[k] - base;
    const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
    float* __restrict__ p = tb.p[k] + base;
    const float* __restrict__ g = tb.g[k] + base;
    float* __restrict__ m = exp_avg + tb.moff[k] + base;
    float* __restrict__ v = exp_avg_sq + tb.moff[k] + base;
    const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;

    const double B1 = state[1] * h.beta1, B2 = state[2] * h.beta2, lr = state[3];
    AdamScalars s;
    s.step_size = (float)(lr / (1.0 - B1));
    s.sbc2 = (float)sqrt(1.0 - B2);
    s.c = h.use_norm ? (float)state[5] : 1.0f;
    s.lrwdf = (float)(lr * h.wd);

    for (int e = threadIdx.x * 4; e < cnt; e += ADAM_THREADS * 4) {
        if (aligned && e + 4 <= cnt) {
            float4 pp = ldg4(p + e), mm = ldg4(m + e), vv = ldg4(v + e);
            const float4 gg = ldg4(g + e);
            adam_element(pp.x, gg.x, mm.x, vv.x, h, s);
            adam_element(pp.y, gg.y, mm.y, vv.y, h, s);
            adam_element(pp.z, gg.z, mm.z, vv.z, h, s);
            adam_element(pp.w, gg.w, mm.w, vv.w, h, s);
            stg4(p + e, pp); stg4(m + e, mm); stg4(v + e, vv);
        } else {                                                 // a view at a 4- or 8-byte offset, a scalar, a tensor's last 1..3 elements
            const int end = e + 4 < cnt ? e + 4 : cnt;
            for (int i = e; i < end; ++i) {
                float pp = p[i], mm = m[i], vv = v[i];
                adam_element(pp, g[i], mm, vv, h, s);
                p[i] = pp; m[i] = mm; v[i] = vv;
            }
        }
    }
}

// Closing pass: one wave, lane 0.  A skipped step leaves t and the powers alone and counts itself; without the norm the slots it would
// have written say so (norm unknown = NaN, coefficient 1, flag 0).
__global__ __launch_bounds__(64)
void adam_close_kernel(double* __restrict__ state, double beta1, double beta2, int use_norm, int skip)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    if (skip && state[7] != 0.0) {
        state[6] += 1.0;
    } else {
        state[0] += 1.0;
        state[1] = state[1] * beta1;
        state[2] = state[2] * beta2;
    }
    if (!use_norm) { state[4] = __builtin_nan(""); state[5] = 1.0; state[7] = 0.0; }
}

// partial[workgroup] = sum of g*g over the workgroup's chunk.  Thread t owns the quads t, t + 256, ... of the chunk and adds their
// elements one by one in index order; the 16-byte and the scalar load path feed the same additions.
__global__ __launch_bounds__(ADAM_THREADS)
void grad_sq_kernel(const AdamTable tb, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int bid = blockIdx.x, k = table_find(tb, bid);
    const long long base = (long long)(bid - tb.cstart[k]) * ADAM_CHUNK;
    const long long left = tb.n[k] - base;
    const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
    const float* __restrict__ g = tb.g[k] + base;
    const bool aligned = (((uintptr_t)g) & 15) == 0;
    double acc = 0.0;
    for (int e = threadIdx.x * 4; e < cnt; e += ADAM_THREADS * 4) {
        if (aligned && e + 4 <= cnt) {
            const float4 x = ldg4(g + e);
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        } else {
            const int end = e + 4 < cnt ? e + 4 : cnt;
            for (int i = e; i < end; ++i) { const double x = (double)g[i]; acc += x * x; }
        }
    }
    const double s = block_sum_f64_fixed(acc, red);
    if (threadIdx.x == 0) partial[bid] = s;
}

// One workgroup: thread t adds the partials t, t + 256, ... in order, then the same fixed tree.  state[4] = norm, state[5] = the clip
// coefficient of torch's clip_grad_norm_ rounded to fp32 (1 when max_norm < 0; a NaN norm gives a NaN coefficient, as there),
// state[7] = 1 when the sum is inf or NaN.
__global__ __launch_bounds__(ADAM_THREADS)
void grad_norm_finalize_kernel(const double* __restrict__ partial, int np, double max_norm, double* __restrict__ state)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += ADAM_THREADS) acc += partial[i];
    const double sum = block_sum_f64_fixed(acc, red);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(sum);
    float c = 1.0f;
    if (max_norm >= 0.0) {
        const double q = max_norm / (norm + 1e-6);
        c = (float)(q < 1.0 || q != q ? q : 1.0);
    }
    state[4] = norm;
    state[5] = (double)c;
    state[7] = sum < (double)INFINITY ? 0.0 : 1.0;               // (a NaN sum compares false)
}

// Fills tables of up to ADAM_CAP non-empty tensors from position *next of the caller's arrays; returns the launch's workgroup count
// (0: nothing left), or -1 if it does not fit an int.
static int fill_table(AdamTable& tb, float* const* param, const float* const* grad, const int64_t* numel, const int64_t* moff, int n, int* next)
{
    tb.nt = 0;
    long long chunks = 0;
    int i = *next;
    for (; i < n && tb.nt < ADAM_CAP; ++i) {
        if (numel[i] == 0) continue;
        const int k = tb.nt++;
        tb.p[k] = param ? param[i] : nullptr;
        tb.g[k] = grad[i];
        tb.moff[k] = moff ? moff[i] : 0;
        tb.n[k] = numel[i];
        tb.cstart[k] = (int)chunks;
        chunks += (numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (chunks > 0x7fffffff) return -1;
    }
    tb.cstart[tb.nt] = (int)chunks;
    *next = i;
    return (int)chunks;
}

static long long total_chunks(const int64_t* numel, int n)
{
    long long c = 0;
    for (int i = 0; i < n; ++i) c += (numel[i] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return c;
}

static bool table_ok(const void* const* a, const void* const* b, const int64_t* numel, int n)
{
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return false;
        if (numel[i] > 0 && ((a && a[i] == nullptr) || b[i] == nullptr)) return false;
    }
    return true;
}

}  // namespace smin

using namespace smin;

extern "C" size_t smin_adam_ws_bytes(int64_t total_numel, int n)
{
    if (total_numel < 0 || n < 0) return 0;
    // a tensor of numel elements has at most numel / CHUNK + 1 chunks
    return (((size_t)(total_numel / ADAM_CHUNK) + (size_t)n + 1) * sizeof(double) + 255) & ~(size_t)255;
}

extern "C" int smin_grad_norm(void* stream, const float* const* grad, const int64_t* numel, int n, double max_norm, double* state,
                              void* ws, size_t ws_bytes)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(n >= 0);
    SMIN_REQUIRE(n == 0 || (grad != nullptr && numel != nullptr));
    SMIN_REQUIRE(table_ok(nullptr, (const void* const*)grad, numel, n));
    SMIN_REQUIRE(max_norm == max_norm);
    const long long np = total_chunks(numel, n);
    if (np == 0) return 0;
    SMIN_REQUIRE(np <= 0x7fffffff && state != nullptr && ws != nullptr && ws_bytes >= (size_t)np * sizeof(double));
    double* partial = (double*)ws;
    AdamTable tb;
    int next = 0, done = 0;
    for (;;) {
        const int wgs = fill_table(tb, nullptr, grad, numel, nullptr, n, &next);
        SMIN_REQUIRE(wgs >= 0);
        if (wgs == 0) break;
        hipLaunchKernelGGL(grad_sq_kernel, dim3(wgs), dim3(ADAM_THREADS), 0, st, tb, partial + done);
        SMIN_LAUNCH_CHECK();
        done += wgs;
    }
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, partial, (int)np, max_norm, state);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_adam_step(void* stream, float* const* param, const float* const* grad, const int64_t* numel, const int64_t* moment_offset,
                              int n, float* exp_avg, float* exp_avg_sq, double* state, double beta1, double beta2, double eps,
                              double weight_decay, int decoupled, int skip_nonfinite, const void* norm_ws)
{
    hipStream_t st = (hipStream_t)stream;
    SMIN_REQUIRE(n >= 0);
    SMIN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    SMIN_REQUIRE(eps >= 0.0 && weight_decay >= 0.0);
    SMIN_REQUIRE(n == 0 || (param != nullptr && grad != nullptr && numel != nullptr && moment_offset != nullptr));
    SMIN_REQUIRE(table_ok((const void* const*)param, (const void* const*)grad, numel, n));
    for (int i = 0; i < n; ++i) SMIN_REQUIRE(moment_offset[i] >= 0);
    SMIN_REQUIRE(!skip_nonfinite || norm_ws != nullptr);            // the guard reads the norm's flag
    const long long nc = total_chunks(numel, n);
    if (nc == 0) return 0;
    SMIN_REQUIRE(nc <= 0x7fffffff);
    SMIN_REQUIRE(exp_avg != nullptr && exp_avg_sq != nullptr && state != nullptr);
    AdamHyper h;
    h.beta1 = beta1; h.beta2 = beta2; h.wd = weight_decay;
    h.b1f = (float)beta1; h.omb1f = (float)(1.0 - beta1);
    h.b2f = (float)beta2; h.omb2f = (float)(1.0 - beta2);
    h.epsf = (float)eps; h.wdf = (float)weight_decay;
    h.wd_mode = weight_decay == 0.0 ? 0 : decoupled ? 2 : 1;
    h.use_norm = norm_ws != nullptr;
    h.skip = skip_nonfinite != 0;
    AdamTable tb;
    int next = 0;
    for (;;) {
        const int wgs = fill_table(tb, param, grad, numel, moment_offset, n, &next);
        SMIN_REQUIRE(wgs >= 0);
        if (wgs == 0) break;
        hipLaunchKernelGGL(adam_update_kernel, dim3(wgs), dim3(ADAM_THREADS), 0, st, tb, exp_avg, exp_avg_sq, (const double*)state, h);
        SMIN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(adam_close_kernel, dim3(1), dim3(64), 0, st, state, beta1, beta2, h.use_norm, h.skip);
    SMIN_LAUNCH_CHECK();
    return 0;
}
