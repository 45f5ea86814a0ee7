// Row-sparse training of a word-vector table: the compact gradient of smin_embed_tokens and a lazy Adam step over its rows
// (smin_embed_tokens_bwd_rows / smin_row_adam_step, include/smin_hip.h), and the merge of several such gradients into
// one (smin_row_lists_merge; INTEGRATION.md 3l: described where its kernels start).
//
//   sort     one workgroup: the (id, position) keys of the batch sorted in LDS (embed_sort.h, the dense backward's sort), then the run
//            heads (a valid key whose predecessor holds another id) counted by a prefix scan in the same workgroup: the head of slot s
//            writes ids[s] and start[s]; start[count] = the number of valid keys, ids[s >= count] = -1.
//   rows     one workgroup per slot (grid n, early exit on the device-side count): rows[s] = the sum of the run's rows of dqf in position
//            order -- the additions of sampling.hip's embed_tokens_bwd_kernel, hence the bits of that row of the dense gradient -- and
//            the row's sum of squares in fp64, each thread over its quads in index order, then a fixed tree.
//   sqnorm   one workgroup adds the per-slot sums in a fixed order.  No atomics anywhere, no V * E pass, no host read.
//   update   one workgroup per slot: optimizer.hip's adam_element without weight decay on row ids[s] of table, exp_avg, exp_avg_sq.  Rows not
//            listed are neither read nor written.
//   close    one wave behind the update: step count, running powers of the betas, norm, scale, skipped-step counter and flag.
#include "common.h"
#include "embed_sort.h"
#include "rank_order.h"
#include "smin_hip.h"

namespace smin {

constexpr int SORT_THREADS = 1024;       // the sorting workgroup; each thread then owns four sorted slots
constexpr int SORT_WAVES = SORT_THREADS / 64;
static_assert(4 * SORT_THREADS == EMBED_BWD_MAX, "thread t owns the sorted slots 4t .. 4t + 3");
constexpr int ROWS_THREADS = 256;
static_assert(ROWS_THREADS == 256, "rank_order.h's block helpers are written for four waves");
constexpr int ROW_ADAM_THREADS = 128;    // E = 300: 75 quads, two waves

// Workspace of smin_embed_tokens_bwd_rows for n positions: keys [n] u64 | partial [n] f64 | start [n + 1] i32.
struct RowsWs {
    unsigned long long* keys;
    double* partial;
    int* start;
};
__host__ __device__ inline RowsWs rows_ws(void* ws, int n)
{
    RowsWs w;
    w.keys = reinterpret_cast<unsigned long long*>(ws);
    w.partial = reinterpret_cast<double*>(w.keys + n);
    w.start = reinterpret_cast<int*>(w.partial + n);
    return w;
}

__global__ __launch_bounds__(SORT_THREADS)
void embed_rows_sort_kernel(const int* __restrict__ tokens, int n, int V, unsigned long long* __restrict__ keys, int* __restrict__ start,
                            int* __restrict__ ids, int* __restrict__ count)
{
    __shared__ unsigned long long s[EMBED_BWD_MAX];
    __shared__ int wave_heads[SORT_WAVES], wave_valid[SORT_WAVES];
    embed_sort_keys(tokens, n, V, s);
    // thread t owns the sorted slots 4t .. 4t + 3 (launched with SORT_THREADS threads): its heads and valid keys, then their exclusive prefix
    const int i0 = 4 * (int)threadIdx.x;
    int heads = 0, valid = 0;
    bool head[4];
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + q;
        head[q] = false;
        if (i < n && s[i] != ~0ull) {
            ++valid;
            head[q] = i == 0 || (unsigned)(s[i - 1] >> 32) != (unsigned)(s[i] >> 32);
            heads += head[q];
        }
    }
    int hs = heads, vs = valid;                                       // inclusive scan inside the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const int h = __shfl_up(hs, o), v = __shfl_up(vs, o);
        if (lane >= o) { hs += h; vs += v; }
    }
    if (lane == 63) { wave_heads[wave] = hs; wave_valid[wave] = vs; }
    __syncthreads();
    int hbase = 0, total = 0, nvalid = 0;
    for (int w = 0; w < SORT_WAVES; ++w) {
        if (w < wave) hbase += wave_heads[w];
        total += wave_heads[w];
        nvalid += wave_valid[w];
    }
    int slot = hbase + hs - heads;                                     // heads before slot 4t
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + q;
        if (i < n) keys[i] = s[i];
        if (head[q]) {
            ids[slot] = (int)(unsigned)(s[i] >> 32);
            start[slot] = i;
            ++slot;
        }
    }
    for (int i = total + (int)threadIdx.x; i < n; i += SORT_THREADS) ids[i] = -1;
    if (threadIdx.x == 0) { start[total] = nvalid; count[0] = total; }
}

__global__ __launch_bounds__(ROWS_THREADS)
void embed_rows_kernel(const float* __restrict__ dqf, const unsigned long long* __restrict__ keys, const int* __restrict__ start,
                       const int* __restrict__ count, int E4, float* __restrict__ rows, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int sl = blockIdx.x;
    if (sl >= count[0]) return;
    const int i = start[sl], end = start[sl + 1];
    const size_t E = (size_t)E4 * 4;
    double acc = 0.0;
    for (int c = threadIdx.x; c < E4; c += blockDim.x) {
        float4 v = ldg4(dqf + (size_t)(unsigned)keys[i] * E + 4 * (size_t)c);
        for (int q = i + 1; q < end; ++q) v = f4add(v, ldg4(dqf + (size_t)(unsigned)keys[q] * E + 4 * (size_t)c));
        stg4(rows + (size_t)sl * E + 4 * (size_t)c, v);
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double sum = block_sum_f64_fixed(acc, red);
    if (threadIdx.x == 0) partial[sl] = sum;
}

// thread t adds the slots t, t + 256, ... in order, then the same fixed tree
__global__ __launch_bounds__(ROWS_THREADS)
void embed_rows_sqnorm_kernel(const double* __restrict__ partial, const int* __restrict__ count, double* __restrict__ sqnorm)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int np = count[0];
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += ROWS_THREADS) acc += partial[i];
    const double sum = block_sum_f64_fixed(acc, red);
    if (threadIdx.x == 0) sqnorm[0] = sum;
}

// ---- merge of several row lists of one table (smin_row_lists_merge)
//   rank     one thread per input slot (r, s < c_r): a lower-bound binary search of its id in every list r' gives lt_r' and present_r';
//            merged position = sum of lt_r' + #{r' < r : present_r'}, a run head iff no r' < r holds the id.  The positions of M = sum of
//            c_r elements are a permutation of [0, M): equal ids adjacent, in ascending r.  entry[position] = head | r << 16 | s.
//   scan     one workgroup: exclusive prefix of the head flags over [0, M) in chunks of 4096 with a carried base; the head of slot q
//            writes ids[q] and start[q]; start[count] = M, ids[q >= count] = -1.
//   rows     one workgroup per output slot (grid N, early exit on the device-side count): the run's rows added in entry order (ascending
//            r), scaled, stored, and the row's sum of squares in fp64 as embed_rows_kernel forms it.
//   sqnorm   embed_rows_sqnorm_kernel.
// Every index formed from list contents (an entry's r and s, a position, a run's bounds) is bounded before it is used, so lists that
// break the ordering contract give unspecified rows and no access outside the buffers.
constexpr int MERGE_MAX_LISTS = 16;
constexpr int MERGE_MAX = 65536;         // N = the sum of the lists' capacities: s < 65536 fits an entry's low 16 bits
constexpr int MERGE_RANK_THREADS = 256;
constexpr unsigned MERGE_HEAD = 0x80000000u;

struct MergeLists {                      // by value: 16 * 28 + 4 bytes of kernel arguments
    const int* ids[MERGE_MAX_LISTS];
    const float* rows[MERGE_MAX_LISTS];
    const int* count[MERGE_MAX_LISTS];
    int n[MERGE_MAX_LISTS];              // capacity of list r
    int off[MERGE_MAX_LISTS + 1];        // off[r] = n[0] + .. + n[r - 1]; off[R] = N
};

// Workspace of smin_row_lists_merge for N slots: partial [N] f64 | entry [N] u32 | start [N + 1] i32.
struct MergeWs {
    double* partial;
    unsigned* entry;
    int* start;
};
__host__ __device__ inline MergeWs merge_ws(void* ws, int N)
{
    MergeWs w;
    w.partial = reinterpret_cast<double*>(ws);
    w.entry = reinterpret_cast<unsigned*>(w.partial + N);
    w.start = reinterpret_cast<int*>(w.entry + N);
    return w;
}

// c_r = min(count_r[0], n[r]), never negative; a list of capacity 0 is not read at all
__device__ __forceinline__ int merge_len(const MergeLists& L, int r)
{
    const int cap = L.n[r];
    if (cap <= 0) return 0;
    const int c = L.count[r][0];
    return c < 0 ? 0 : (c > cap ? cap : c);
}

// first index in ids[0 .. c) whose id is not below `id` (c when none): at most 17 steps, every probe inside [0, c)
__device__ __forceinline__ int merge_lower_bound(const int* __restrict__ ids, int c, int id)
{
    int lo = 0, hi = c;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(MERGE_RANK_THREADS)
void merge_rank_kernel(const MergeLists L, int R, int N, unsigned* __restrict__ entry)
{
    const int g = blockIdx.x * MERGE_RANK_THREADS + threadIdx.x;
    if (g >= N) return;
    int r = 0;
    while (r + 1 < R && g >= L.off[r + 1]) ++r;
    const int s = g - L.off[r];
    if (s < 0 || s >= merge_len(L, r)) return;
    const int id = L.ids[r][s];
    int p = 0, before = 0;
    for (int q = 0; q < R; ++q) {
        const int c = merge_len(L, q);
        const int lb = merge_lower_bound(L.ids[q], c, id);
        p += lb;
        if (q < r && lb < c && L.ids[q][lb] == id) ++before;
    }
    p += before;
    if (p < N) entry[p] = (before == 0 ? MERGE_HEAD : 0u) | ((unsigned)r << 16) | (unsigned)s;
}

// the slot of list r an entry names, or -1 for an entry that names none (possible only behind lists that break the contract)
__device__ __forceinline__ int merge_entry_slot(const MergeLists& L, int R, unsigned e, int& r)
{
    r = (int)((e >> 16) & 15u);
    const int s = (int)(e & 0xffffu);
    return (r < R && s < merge_len(L, r)) ? s : -1;
}

__global__ __launch_bounds__(SORT_THREADS)
void merge_scan_kernel(const MergeLists L, int R, int N, const unsigned* __restrict__ entry, int* __restrict__ start, int* __restrict__ ids,
                       int* __restrict__ count)
{
    __shared__ int wave_heads[SORT_WAVES];
    int M = 0;
    for (int r = 0; r < R; ++r) M += merge_len(L, r);
    if (M > N) M = N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carried = 0;                                                  // heads before this chunk
    for (int base = 0; base < M; base += EMBED_BWD_MAX) {             // M is the same in every thread: no divergent barrier
        const int i0 = base + 4 * (int)threadIdx.x;
        int heads = 0, id[4] = {0, 0, 0, 0};
        bool head[4];
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            head[q] = false;
            if (i < M) {
                const unsigned e = entry[i];
                int r;
                const int s = merge_entry_slot(L, R, e, r);
                if ((e & MERGE_HEAD) && s >= 0) { head[q] = true; id[q] = L.ids[r][s]; ++heads; }
            }
        }
        int hs = heads;                                               // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int h = __shfl_up(hs, o);
            if (lane >= o) hs += h;
        }
        if (lane == 63) wave_heads[wave] = hs;
        __syncthreads();
        int hbase = 0, total = 0;
        for (int w = 0; w < SORT_WAVES; ++w) {
            if (w < wave) hbase += wave_heads[w];
            total += wave_heads[w];
        }
        int slot = carried + hbase + hs - heads;                      // heads before position i0: at most i0 < N
        for (int q = 0; q < 4; ++q)
            if (head[q]) {
                ids[slot] = id[q];
                start[slot] = i0 + q;
                ++slot;
            }
        carried += total;
        __syncthreads();                                              // wave_heads is rewritten by the next chunk
    }
    for (int i = carried + (int)threadIdx.x; i < N; i += SORT_THREADS) ids[i] = -1;
    if (threadIdx.x == 0) { start[carried] = M; count[0] = carried; }  // carried <= M <= N: start has N + 1 entries
}

__global__ __launch_bounds__(ROWS_THREADS)
void merge_rows_kernel(const MergeLists L, int R, int N, const unsigned* __restrict__ entry, const int* __restrict__ start,
                       const int* __restrict__ count, const double* __restrict__ scale, int E4, float* __restrict__ rows,
                       double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    __shared__ const float* src[MERGE_MAX_LISTS];
    const int sl = blockIdx.x;
    if (sl >= count[0]) return;
    const size_t E = (size_t)E4 * 4;
    const int i = start[sl];
    int len = start[sl + 1] - i;                                      // a run holds one element per list at most
    if (i < 0 || len < 0) len = 0;
    if (len > R) len = R;
    if (len > N - i) len = N - i;
    if ((int)threadIdx.x < MERGE_MAX_LISTS) {
        const float* p = nullptr;
        if ((int)threadIdx.x < len) {
            int r;
            const int s = merge_entry_slot(L, R, entry[i + (int)threadIdx.x], r);
            if (s >= 0) p = L.rows[r] + (size_t)s * E;
        }
        src[threadIdx.x] = p;
    }
    __syncthreads();
    const bool scaled = scale != nullptr;
    const float cf = scaled ? (float)scale[0] : 1.0f;
    double acc = 0.0;
    for (int c = threadIdx.x; c < E4; c += blockDim.x) {
        float4 v = f4zero();
        bool have = false;
        for (int k = 0; k < len; ++k) {
            if (src[k] == nullptr) continue;
            const float4 x = ldg4(src[k] + 4 * (size_t)c);
            v = have ? f4add(v, x) : x;
            have = true;
        }
        if (scaled) v = f4scale(v, cf);
        stg4(rows + (size_t)sl * E + 4 * (size_t)c, v);
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double sum = block_sum_f64_fixed(acc, red);
    if (threadIdx.x == 0) partial[sl] = sum;
}

// ---- lazy Adam over the listed rows
struct RowAdamHyper {
    double beta1, beta2;
    float b1f, omb1f, b2f, omb2f, epsf;
    int skip;                            // write nothing when the squared norm or the scale is inf or NaN
};

// the scale as the update uses it (cast once to fp32; 1 when none is given) and whether this step is to be skipped
__device__ __forceinline__ bool row_adam_guard(const double* sqnorm, const double* scale, int skip, float& c)
{
    c = scale ? (float)scale[0] : 1.0f;
    if (!skip) return false;
    const bool bad_norm = sqnorm && !(sqnorm[0] < (double)INFINITY);  // (a NaN compares false)
    const bool bad_scale = !(fabsf(c) < INFINITY);
    return bad_norm || bad_scale;
}

struct RowAdamScalars { float step_size, sbc2, c; bool scaled; };

// optimizer.hip's adam_element without weight decay: every fp32 operation rounded on its own
__device__ __forceinline__ void row_adam_element(float& p, float gr, float& m, float& v, const RowAdamHyper& h, const RowAdamScalars& s)
{
#pragma clang fp contract(off)
    const float g = s.scaled ? gr * s.c : gr;
    m = h.b1f * m + h.omb1f * g;
    v = h.b2f * v + (h.omb2f * g) * g;
    p = p - s.step_size * (m / (sqrtf(v) / s.sbc2 + h.epsf));
}

__global__ __launch_bounds__(ROW_ADAM_THREADS)
void row_adam_update_kernel(float* __restrict__ table, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, const int* __restrict__ ids,
                            const float* __restrict__ rows, const int* __restrict__ count, const double* __restrict__ sqnorm, int V, int E4,
                            const double* __restrict__ state, const double* __restrict__ scale, const RowAdamHyper h)
{
#pragma clang fp contract(off)
    const int sl = blockIdx.x;
    if (sl >= count[0]) return;
    float c;
    if (row_adam_guard(sqnorm, scale, h.skip, c)) return;           // table, m and v keep their bits
    const int id = ids[sl];
    if (id < 0 || id >= V) return;
    const double B1 = state[1] * h.beta1, B2 = state[2] * h.beta2, lr = state[3];
    const float step_size = (float)(lr / (1.0 - B1));
    const float sbc2 = (float)sqrt(1.0 - B2);
    const bool scaled = scale != nullptr;
    const size_t E = (size_t)E4 * 4, row = (size_t)id * E, src = (size_t)sl * E;
    const RowAdamScalars sc{step_size, sbc2, c, scaled};
    for (int q = threadIdx.x; q < E4; q += blockDim.x) {
        const size_t e = row + 4 * (size_t)q;
        float4 pp = ldg4(table + e), mm = ldg4(exp_avg + e), vv = ldg4(exp_avg_sq + e);
        const float4 gg = ldg4(rows + src + 4 * (size_t)q);
        row_adam_element(pp.x, gg.x, mm.x, vv.x, h, sc);
        row_adam_element(pp.y, gg.y, mm.y, vv.y, h, sc);
        row_adam_element(pp.z, gg.z, mm.z, vv.z, h, sc);
        row_adam_element(pp.w, gg.w, mm.w, vv.w, h, sc);
        stg4(table + e, pp); stg4(exp_avg + e, mm); stg4(exp_avg_sq + e, vv);
    }
}

// Closing pass: one wave, lane 0.  A skipped step leaves t and the powers alone and counts itself.
__global__ __launch_bounds__(64)
void row_adam_close_kernel(double* __restrict__ state, const double* __restrict__ sqnorm, const double* __restrict__ scale, double beta1,
                           double beta2, int skip)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    float c;
    const bool skipped = row_adam_guard(sqnorm, scale, skip, c);
    if (skipped) {
        state[6] += 1.0;
    } else {
        state[0] += 1.0;
        state[1] = state[1] * beta1;
        state[2] = state[2] * beta2;
    }
    const bool bad = (sqnorm && !(sqnorm[0] < (double)INFINITY)) || !(fabsf(c) < INFINITY);
    state[4] = sqnorm ? sqrt(sqnorm[0]) : __builtin_nan("");
    state[5] = (double)c;
    state[7] = bad ? 1.0 : 0.0;
}

}  // namespace smin

using namespace smin;

extern "C" size_t smin_embed_tokens_bwd_rows_workspace_bytes(int B, int Nq)
{
    const size_t n = (size_t)(B > 0 ? B : 0) * (size_t)(Nq > 0 ? Nq : 0);
    return (sizeof(unsigned long long) + sizeof(double)) * n + sizeof(int) * (n + 1) + 256;
}

extern "C" int smin_embed_tokens_bwd_rows(void* stream, const int32_t* tokens, const float* dqf, int B, int Nq, int V, int E, int32_t* ids,
                                          float* rows, int32_t* count, double* sqnorm, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(B >= 0 && Nq >= 1 && V >= 1 && E >= 4 && E % 4 == 0 && (long long)B * Nq <= EMBED_BWD_MAX);
    SMIN_REQUIRE(count != nullptr && sqnorm != nullptr && ws != nullptr && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)sqnorm & 7) == 0);
    SMIN_REQUIRE(ws_bytes >= smin_embed_tokens_bwd_rows_workspace_bytes(B, Nq));
    const int n = B * Nq;
    SMIN_REQUIRE(n == 0 || (tokens != nullptr && dqf != nullptr && ids != nullptr && rows != nullptr));
    SMIN_REQUIRE(((uintptr_t)dqf & 15) == 0 && ((uintptr_t)rows & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    const RowsWs w = rows_ws(ws, n);
    hipLaunchKernelGGL(embed_rows_sort_kernel, dim3(1), dim3(SORT_THREADS), 0, st, tokens, n, V, w.keys, w.start, ids, count);
    SMIN_LAUNCH_CHECK();
    if (n > 0) {
        hipLaunchKernelGGL(embed_rows_kernel, dim3(n), dim3(ROWS_THREADS), 0, st, dqf, (const unsigned long long*)w.keys, (const int*)w.start,
                           (const int*)count, E / 4, rows, w.partial);
        SMIN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(embed_rows_sqnorm_kernel, dim3(1), dim3(ROWS_THREADS), 0, st, (const double*)w.partial, (const int*)count, sqnorm);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_row_lists_merge_workspace_bytes(int R, int N)
{
    (void)R;
    const size_t n = (size_t)(N > 0 ? N : 0);
    return (sizeof(double) + sizeof(unsigned)) * n + sizeof(int) * (n + 1) + 256;
}

extern "C" int smin_row_lists_merge(void* stream, const int32_t* const* ids, const float* const* rows, const int32_t* const* count, const int* n,
                                    int R, int V, int E, const double* scale, int32_t* out_ids, float* out_rows, int32_t* out_count,
                                    double* out_sqnorm, void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(R >= 1 && R <= MERGE_MAX_LISTS && V >= 1 && E >= 4 && E % 4 == 0 && n != nullptr);
    MergeLists L;
    long long total = 0;
    for (int r = 0; r < MERGE_MAX_LISTS; ++r) {
        L.ids[r] = nullptr; L.rows[r] = nullptr; L.count[r] = nullptr; L.n[r] = 0;
        L.off[r] = (int)total;
        if (r < R) {
            SMIN_REQUIRE(n[r] >= 0 && n[r] <= MERGE_MAX);
            L.n[r] = n[r];
            total += n[r];
            SMIN_REQUIRE(total <= MERGE_MAX);
        }
    }
    const int N = (int)total;
    L.off[MERGE_MAX_LISTS] = N;
    SMIN_REQUIRE(((uintptr_t)scale & 7) == 0 && ((uintptr_t)out_sqnorm & 7) == 0 && ((uintptr_t)out_rows & 15) == 0 && ((uintptr_t)ws & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                                                     // nothing listed: count = 0 and sqnorm = 0 where they are asked for
        if (out_count && hipMemsetAsync(out_count, 0, sizeof(int32_t), st) != hipSuccess) return (int)hipGetLastError();
        if (out_sqnorm && hipMemsetAsync(out_sqnorm, 0, sizeof(double), st) != hipSuccess) return (int)hipGetLastError();
        return 0;
    }
    SMIN_REQUIRE(ids != nullptr && rows != nullptr && count != nullptr);
    SMIN_REQUIRE(out_ids != nullptr && out_rows != nullptr && out_count != nullptr && out_sqnorm != nullptr && ws != nullptr);
    SMIN_REQUIRE(ws_bytes >= smin_row_lists_merge_workspace_bytes(R, N));
    for (int r = 0; r < R; ++r) {
        if (n[r] == 0) continue;                                      // a list without capacity is never read
        SMIN_REQUIRE(ids[r] != nullptr && rows[r] != nullptr && count[r] != nullptr && ((uintptr_t)rows[r] & 15) == 0);
        L.ids[r] = ids[r]; L.rows[r] = rows[r]; L.count[r] = count[r];
    }
    const MergeWs w = merge_ws(ws, N);
    hipLaunchKernelGGL(merge_rank_kernel, dim3(cdiv(N, MERGE_RANK_THREADS)), dim3(MERGE_RANK_THREADS), 0, st, L, R, N, w.entry);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_scan_kernel, dim3(1), dim3(SORT_THREADS), 0, st, L, R, N, (const unsigned*)w.entry, w.start, out_ids, out_count);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_rows_kernel, dim3(N), dim3(ROWS_THREADS), 0, st, L, R, N, (const unsigned*)w.entry, (const int*)w.start,
                       (const int*)out_count, scale, E / 4, out_rows, w.partial);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_rows_sqnorm_kernel, dim3(1), dim3(ROWS_THREADS), 0, st, (const double*)w.partial, (const int*)out_count, out_sqnorm);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_row_adam_step(void* stream, float* table, float* exp_avg, float* exp_avg_sq, const int32_t* ids, const float* rows,
                                  const int32_t* count, const double* sqnorm, int n, int V, int E, double* state, const double* scale,
                                  double beta1, double beta2, double eps, int skip_nonfinite)
{
    SMIN_REQUIRE(n >= 0 && n <= MERGE_MAX && V >= 1 && E >= 4 && E % 4 == 0);   // a merged list may hold 16 lists' slots
    SMIN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0);
    SMIN_REQUIRE(state != nullptr && ((uintptr_t)state & 7) == 0 && ((uintptr_t)scale & 7) == 0 && ((uintptr_t)sqnorm & 7) == 0);
    SMIN_REQUIRE(n == 0 || (table != nullptr && exp_avg != nullptr && exp_avg_sq != nullptr && ids != nullptr && rows != nullptr && count != nullptr));
    SMIN_REQUIRE(((((uintptr_t)table) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq) | ((uintptr_t)rows)) & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    RowAdamHyper h;
    h.beta1 = beta1; h.beta2 = beta2;
    h.b1f = (float)beta1; h.omb1f = (float)(1.0 - beta1);
    h.b2f = (float)beta2; h.omb2f = (float)(1.0 - beta2);
    h.epsf = (float)eps;
    h.skip = skip_nonfinite != 0;
    if (n > 0) {
        hipLaunchKernelGGL(row_adam_update_kernel, dim3(n), dim3(ROW_ADAM_THREADS), 0, st, table, exp_avg, exp_avg_sq, ids, rows, count, sqnorm,
                           V, E / 4, (const double*)state, scale, h);
        SMIN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(row_adam_close_kernel, dim3(1), dim3(64), 0, st, state, sqnorm, scale, beta1, beta2, h.skip);
    SMIN_LAUNCH_CHECK();
    return 0;
}
