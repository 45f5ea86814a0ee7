// Per-sample input transforms of the reference's loader on the device: the clip resampling of each video's raw feature rows
// (dataset.py:40-74, get_fixed_length_features) and the word-vector lookup of each query (dataset.py:32-38, get_query_features).
//
// smin_sample_clips -- sample b owns raw rows offsets[b] .. offsets[b+1] (n = their count), output (B, T, Din), nfeats = min(n, T).
//   pick (mode 0, the reference), all in double:
//     stride = 1 if n <= T else n / T;  delta = (spos + stride) - spos  (numpy arange's fill step);
//     idx_t  = rint(spos + t * delta)  (round half to even, np.round), for t < min(n, T);  out[b, t] = raw[offsets[b] + idx_t].
//     spos is clamped into the range the reference draws from, [0, int(r + 1)) with r = stride - 0.5, minus 1 when r is integral
//     (dataset.py:45-49), so no spos reads outside the sample.
//   mean (mode 1, spos = 0): n <= T as pick; n > T: out[b, t] = mean of raw rows [a_t, a_{t+1}), a_t = rint(t * n / T) in double,
//     a_T = n; fp32 sum in ascending row order, then one fp32 division by the row count.
//   rows t >= min(n, T) are zero.  Memory: one copy (pick) or one streaming read (mean); float4 along Din, 64-bit addressing.
// smin_sample_windows -- the same kernel (a template on how a sample finds its rows) for samples that each own an arbitrary row
//   range row_begin[w] .. row_begin[w] + len[w] of raw (ranges may overlap or repeat; nothing is copied); spos = 0 (eval split).
// smin_embed_tokens -- out[b, w] = table[tokens[b, w]] (zero row for an id outside [0, V)), mask = 0 <= id < pad_id, qlen = sum mask.
// Backward (deterministic, no atomics): smin_sample_clips_bwd gives each raw row the sum, in ascending t, of the output rows that read it
// (pick) or its window's output row over the window's row count (mean); smin_embed_tokens_bwd sorts the (id, position) pairs of the
// batch in one workgroup, then one workgroup per distinct id adds its positions' rows in ascending position order.
#include "common.h"
#include "embed_sort.h"
#include "smin_hip.h"

namespace smin {

constexpr int SAMPLE_ROWS = 16;          // output rows per workgroup

// How output sample b finds its raw rows: base = its first row, n = its row count.
struct OffsetRows {                      // smin_sample_clips: consecutive samples, rows offsets[b] .. offsets[b+1]
    const long long* offsets;
    __device__ __forceinline__ void operator()(int b, long long& base, long long& n) const
    {
        base = offsets[b];
        n = max(offsets[b + 1] - base, 0LL);
    }
};

struct RangeRows {                       // smin_sample_windows: rows begin[b] .. begin[b] + len[b] (ranges may overlap and repeat)
    const long long* begin;
    const int* len;
    __device__ __forceinline__ void operator()(int b, long long& base, long long& n) const
    {
        base = begin[b];
        n = max((long long)len[b], 0LL);
    }
};

template <typename Rows>
__global__ __launch_bounds__(256)
void sample_clips_kernel(const float* __restrict__ raw, Rows rows_of, const int* __restrict__ spos_in, int mode,
                         int T, int D4, float* __restrict__ out, int* __restrict__ nfeats)
{
    __shared__ long long s_first[SAMPLE_ROWS];    // first raw row (absolute) of output row t, or -1: a zero row
    __shared__ int s_count[SAMPLE_ROWS];          // rows averaged (1 = a copy)
    const int b = blockIdx.y, t0 = blockIdx.x * SAMPLE_ROWS;
    long long base, n;
    rows_of(b, base, n);
    const int nf = (int)min(n, (long long)T);
    if (threadIdx.x < SAMPLE_ROWS) {
        const int t = t0 + threadIdx.x;
        long long first = -1;
        int cnt = 1;
        if (t < nf) {
            if (n <= T) {
                first = t;
            } else if (mode == 0) {
                const double stride = (double)n / (double)T;
                double r = stride - 0.5;
                if (r == floor(r)) r -= 1.0;
                const long long hi = (long long)(r + 1.0) - 1;                 // largest spos np.random.randint(0, r + 1) draws
                const long long sp = spos_in ? min(max((long long)spos_in[b], 0LL), hi) : 0;
                const double s = (double)sp;
                const double delta = __dsub_rn(__dadd_rn(s, stride), s);
                const long long idx = (long long)rint(__dadd_rn(s, __dmul_rn((double)t, delta)));
                first = min(max(idx, 0LL), n - 1);
            } else {
                const long long a0 = (long long)rint(__ddiv_rn(__dmul_rn((double)t, (double)n), (double)T));
                const long long a1 = t + 1 == T ? n : (long long)rint(__ddiv_rn(__dmul_rn((double)(t + 1), (double)n), (double)T));
                first = a0;
                cnt = (int)(a1 - a0);
            }
        }
        s_first[threadIdx.x] = first < 0 ? -1 : base + first;
        s_count[threadIdx.x] = cnt;
        if (blockIdx.x == 0 && threadIdx.x == 0) nfeats[b] = nf;
    }
    __syncthreads();
    const int rows = min(SAMPLE_ROWS, T - t0);
    const size_t Din = (size_t)D4 * 4;
    for (int k = threadIdx.x; k < rows * D4; k += blockDim.x) {
        const int r = k / D4, c = k - r * D4;
        const long long first = s_first[r];
        float4 v = f4zero();
        if (first >= 0) {
            const float* src = raw + (size_t)first * Din + 4 * (size_t)c;
            v = ldg4(src);
            const int cnt = s_count[r];
            if (cnt > 1) {
                for (int q = 1; q < cnt; ++q) v = f4add(v, ldg4(src + (size_t)q * Din));
                const float fc = (float)cnt;
                v = make_float4(v.x / fc, v.y / fc, v.z / fc, v.w / fc);
            }
        }
        stg4(out + ((size_t)b * T + t0 + r) * Din + 4 * (size_t)c, v);
    }
}

__global__ __launch_bounds__(256)
void embed_tokens_kernel(const int* __restrict__ tokens, const float* __restrict__ table, int V, int E4, int Nq, int pad_id,
                         float* __restrict__ out, uint8_t* __restrict__ mask, int* __restrict__ qlen)
{
    const int b = blockIdx.x;
    const int* tok = tokens + (size_t)b * Nq;
    if (threadIdx.x < 64) {                                                   // wave 0: mask and length
        int n = 0;
        for (int w0 = 0; w0 < Nq; w0 += 64) {
            const int w = w0 + threadIdx.x;
            bool m = false;
            if (w < Nq) {
                const int id = tok[w];
                m = id >= 0 && id < V && id < pad_id;
                mask[(size_t)b * Nq + w] = m;
            }
            n += __popcll(__ballot(m));
        }
        if (threadIdx.x == 0) qlen[b] = n;
    }
    const size_t E = (size_t)E4 * 4;
    for (int k = threadIdx.x; k < Nq * E4; k += blockDim.x) {
        const int w = k / E4, c = k - w * E4;
        const int id = tok[w];
        const float4 v = (id >= 0 && id < V) ? ldg4(table + (size_t)id * E + 4 * (size_t)c) : f4zero();
        stg4(out + ((size_t)b * Nq + w) * E + 4 * (size_t)c, v);
    }
}


// ---- backward of smin_sample_clips
// The raw row the forward reads for output row t < nf of a sample (the first row of t's window in mean mode); non-decreasing in t.
__device__ __forceinline__ long long clip_source(long long t, long long n, int T, int mode, long long sp, double stride, double delta)
{
    if (n <= T) return t;
    if (mode == 0) {
        const long long idx = (long long)rint(__dadd_rn((double)sp, __dmul_rn((double)t, delta)));
        return min(max(idx, 0LL), n - 1);
    }
    return (long long)rint(__ddiv_rn(__dmul_rn((double)t, (double)n), (double)T));
}

// draw[r] for raw rows r of one 16-row block: sample b by binary search over offsets, then the output rows [t_lo, t_hi) that read row
// j = r - offsets[b] by binary search over t (clip_source is monotone): pick -> every t with source j; mean (n > T) -> the window t
// with a_t <= j < a_{t+1}, divided by cnt_t.  Rows read by no output row (and rows outside every sample) are zero.
__global__ __launch_bounds__(256)
void sample_clips_bwd_kernel(const float* __restrict__ dout, const long long* __restrict__ offsets, const int* __restrict__ spos_in, int mode,
                             int B, int T, int D4, long long rows, float* __restrict__ draw)
{
    __shared__ long long s_src[SAMPLE_ROWS];      // first output row (absolute, b * T + t_lo) or -1
    __shared__ int s_count[SAMPLE_ROWS];          // output rows summed
    __shared__ int s_div[SAMPLE_ROWS];            // cnt_t, the divisor of the row's window (mean), or 1
    const long long r0 = (long long)blockIdx.x * SAMPLE_ROWS;
    if (threadIdx.x < SAMPLE_ROWS) {
        const long long r = r0 + threadIdx.x;
        long long src = -1;
        int cnt = 0, div = 1;
        if (r < rows && B > 0 && r >= offsets[0] && r < offsets[B]) {
            int lo = 0, hi = B - 1;                                        // largest b with offsets[b] <= r
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
            }
            const int b = lo;
            const long long base = offsets[b], n = offsets[b + 1] - base, j = r - base;
            const int nf = (int)min(n, (long long)T);
            const double stride = n <= T ? 1.0 : (double)n / (double)T;
            long long sp = 0;
            if (mode == 0 && n > T) {
                double rr = stride - 0.5;
                if (rr == floor(rr)) rr -= 1.0;
                const long long shi = (long long)(rr + 1.0) - 1;
                sp = spos_in ? min(max((long long)spos_in[b], 0LL), shi) : 0;
            }
            const double delta = __dsub_rn(__dadd_rn((double)sp, stride), (double)sp);
            auto first_above = [&](long long v) {                          // smallest t in [0, nf] with clip_source(t) > v
                int a = 0, z = nf;
                while (a < z) {
                    const int mid = (a + z) >> 1;
                    if (clip_source(mid, n, T, mode, sp, stride, delta) > v) z = mid; else a = mid + 1;
                }
                return a;
            };
            if (mode == 1 && n > T) {
                const int t = first_above(j) - 1;                          // a_0 = 0 <= j < n = a_T
                const long long a1 = t + 1 == T ? n : clip_source(t + 1, n, T, mode, sp, stride, delta);
                src = (long long)b * T + t;
                cnt = 1;
                div = (int)(a1 - clip_source(t, n, T, mode, sp, stride, delta));
            } else {
                const int t_lo = first_above(j - 1), t_hi = first_above(j);
                if (t_hi > t_lo) { src = (long long)b * T + t_lo; cnt = t_hi - t_lo; }
            }
        }
        s_src[threadIdx.x] = src;
        s_count[threadIdx.x] = cnt;
        s_div[threadIdx.x] = div;
    }
    __syncthreads();
    const int nrows = (int)min((long long)SAMPLE_ROWS, rows - r0);
    const size_t Din = (size_t)D4 * 4;
    for (int k = threadIdx.x; k < nrows * D4; k += blockDim.x) {
        const int q = k / D4, c = k - q * D4;
        const long long src = s_src[q];
        float4 v = f4zero();
        if (src >= 0) {
            const float* g = dout + (size_t)src * Din + 4 * (size_t)c;
            v = ldg4(g);
            for (int u = 1; u < s_count[q]; ++u) v = f4add(v, ldg4(g + (size_t)u * Din));     // ascending t
            if (s_div[q] > 1) {                                            // as the forward's division: d(v / cnt) = dv / cnt
                const float fc = (float)s_div[q];
                v = make_float4(v.x / fc, v.y / fc, v.z / fc, v.w / fc);
            }
        }
        stg4(draw + (size_t)(r0 + q) * Din + 4 * (size_t)c, v);
    }
}

// ---- backward of smin_embed_tokens
// keys[i] = (id << 32 | position) sorted ascending (embed_sort.h, one workgroup); positions with an id outside [0, V) are given the
// largest key and never read.  Equal ids end up adjacent, in ascending position order.
__global__ __launch_bounds__(1024)
void embed_tokens_sort_kernel(const int* __restrict__ tokens, int n, int V, unsigned long long* __restrict__ keys)
{
    __shared__ unsigned long long s[EMBED_BWD_MAX];
    embed_sort_keys(tokens, n, V, s);
    for (int i = threadIdx.x; i < n; i += blockDim.x) keys[i] = s[i];
}

// one workgroup per sorted slot i; the first slot of each id's run writes dtable[id] = sum of the run's rows of dqf in position order
__global__ __launch_bounds__(256)
void embed_tokens_bwd_kernel(const float* __restrict__ dqf, const unsigned long long* __restrict__ keys, int n, int E4, float* __restrict__ dtable)
{
    const int i = blockIdx.x;
    const unsigned long long k = keys[i];
    if (k == ~0ull) return;
    const unsigned id = (unsigned)(k >> 32);
    if (i > 0 && (unsigned)(keys[i - 1] >> 32) == id) return;
    int end = i + 1;
    while (end < n && keys[end] != ~0ull && (unsigned)(keys[end] >> 32) == id) ++end;
    const size_t E = (size_t)E4 * 4;
    for (int c = threadIdx.x; c < E4; c += blockDim.x) {
        float4 v = ldg4(dqf + (size_t)(unsigned)keys[i] * E + 4 * (size_t)c);
        for (int q = i + 1; q < end; ++q) v = f4add(v, ldg4(dqf + (size_t)(unsigned)keys[q] * E + 4 * (size_t)c));
        stg4(dtable + (size_t)id * E + 4 * (size_t)c, v);
    }
}

}  // namespace smin

extern "C" int smin_sample_clips(void* stream, const float* raw, const int64_t* offsets, const int32_t* spos, int B, int T, int Din, int mode,
                                 float* video_features, int32_t* nfeats)
{
    SMIN_REQUIRE(B >= 0 && B <= 65535 && T >= 1 && Din >= 4 && Din % 4 == 0 && (mode == 0 || (mode == 1 && spos == nullptr)));
    SMIN_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)video_features & 15) == 0);
    if (B == 0) return 0;
    hipLaunchKernelGGL(smin::sample_clips_kernel<smin::OffsetRows>, dim3(cdiv(T, smin::SAMPLE_ROWS), B), dim3(256), 0, (hipStream_t)stream, raw,
                       smin::OffsetRows{(const long long*)offsets}, spos, mode, T, Din / 4, video_features, nfeats);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_sample_windows(void* stream, const float* raw, const int64_t* row_begin, const int32_t* len, int W, int T, int Din, int mode,
                                   float* video_features, int32_t* nfeats)
{
    SMIN_REQUIRE(W >= 0 && W <= 65535 && T >= 1 && Din >= 4 && Din % 4 == 0 && (mode == 0 || mode == 1));
    SMIN_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)video_features & 15) == 0);
    if (W == 0) return 0;
    SMIN_REQUIRE(raw != nullptr && row_begin != nullptr && len != nullptr && video_features != nullptr && nfeats != nullptr);
    hipLaunchKernelGGL(smin::sample_clips_kernel<smin::RangeRows>, dim3(cdiv(T, smin::SAMPLE_ROWS), W), dim3(256), 0, (hipStream_t)stream, raw,
                       smin::RangeRows{(const long long*)row_begin, len}, nullptr, mode, T, Din / 4, video_features, nfeats);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_embed_tokens(void* stream, const int32_t* tokens, const float* table, int B, int Nq, int V, int E, int pad_id,
                                 float* query_features, uint8_t* query_mask, int32_t* qlen)
{
    SMIN_REQUIRE(B >= 0 && Nq >= 1 && V >= 1 && E >= 4 && E % 4 == 0);
    SMIN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)query_features & 15) == 0);
    if (B == 0) return 0;
    hipLaunchKernelGGL(smin::embed_tokens_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tokens, table, V, E / 4, Nq, pad_id,
                       query_features, query_mask, qlen);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_sample_clips_bwd(void* stream, const float* dout, const int64_t* offsets, const int32_t* spos, int B, int T, int Din, int mode,
                                     int64_t rows, float* draw)
{
    SMIN_REQUIRE(B >= 0 && B <= 65535 && T >= 1 && Din >= 4 && Din % 4 == 0 && rows >= 0 && (mode == 0 || (mode == 1 && spos == nullptr)));
    SMIN_REQUIRE(((uintptr_t)dout & 15) == 0 && ((uintptr_t)draw & 15) == 0);
    const long long blocks = (rows + smin::SAMPLE_ROWS - 1) / smin::SAMPLE_ROWS;
    SMIN_REQUIRE(blocks <= 0x7fffffffLL);
    if (rows == 0) return 0;
    hipLaunchKernelGGL(smin::sample_clips_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dout, (const long long*)offsets, spos,
                       mode, B, T, Din / 4, (long long)rows, draw);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t smin_embed_tokens_bwd_workspace_bytes(int B, int Nq)
{
    return sizeof(unsigned long long) * (size_t)(B > 0 ? B : 0) * (size_t)(Nq > 0 ? Nq : 0) + 256;
}

extern "C" int smin_embed_tokens_bwd(void* stream, const int32_t* tokens, const float* dqf, int B, int Nq, int V, int E, float* dtable,
                                     void* ws, size_t ws_bytes)
{
    SMIN_REQUIRE(B >= 0 && Nq >= 1 && V >= 1 && E >= 4 && E % 4 == 0 && (long long)B * Nq <= smin::EMBED_BWD_MAX);
    SMIN_REQUIRE(((uintptr_t)dqf & 15) == 0 && ((uintptr_t)dtable & 15) == 0 && ((uintptr_t)ws & 7) == 0);
    SMIN_REQUIRE(ws_bytes >= smin_embed_tokens_bwd_workspace_bytes(B, Nq));
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(dtable, 0, sizeof(float) * (size_t)V * E, st);      // rows no token touches
    if (e != hipSuccess) return (int)e;
    const int n = B * Nq;
    if (n == 0) return 0;
    auto* keys = reinterpret_cast<unsigned long long*>(ws);
    hipLaunchKernelGGL(smin::embed_tokens_sort_kernel, dim3(1), dim3(1024), 0, st, tokens, n, V, keys);
    SMIN_LAUNCH_CHECK();
    hipLaunchKernelGGL(smin::embed_tokens_bwd_kernel, dim3(n), dim3(256), 0, st, dqf, keys, n, E / 4, dtable);
    SMIN_LAUNCH_CHECK();
    return 0;
}
