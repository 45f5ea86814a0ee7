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
// smin_embed_tokens -- out[b, w] = table[tokens[b, w]] (zero row for an id outside [0, V)), mask = 0 <= id < pad_id, qlen = sum mask.
#include "common.h"
#include "smin_hip.h"

namespace smin {

constexpr int SAMPLE_ROWS = 16;          // output rows per workgroup

__global__ __launch_bounds__(256)
void sample_clips_kernel(const float* __restrict__ raw, const long long* __restrict__ offsets, const int* __restrict__ spos_in, int mode,
                         int T, int D4, float* __restrict__ out, int* __restrict__ nfeats)
{
    __shared__ long long s_first[SAMPLE_ROWS];    // first raw row (absolute) of output row t, or -1: a zero row
    __shared__ int s_count[SAMPLE_ROWS];          // rows averaged (1 = a copy)
    const int b = blockIdx.y, t0 = blockIdx.x * SAMPLE_ROWS;
    const long long base = offsets[b];
    const long long n = max(offsets[b + 1] - base, 0LL);
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

}  // namespace smin

extern "C" int smin_sample_clips(void* stream, const float* raw, const int64_t* offsets, const int32_t* spos, int B, int T, int Din, int mode,
                                 float* video_features, int32_t* nfeats)
{
    SMIN_REQUIRE(B >= 0 && B <= 65535 && T >= 1 && Din >= 4 && Din % 4 == 0 && (mode == 0 || (mode == 1 && spos == nullptr)));
    SMIN_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)video_features & 15) == 0);
    if (B == 0) return 0;
    hipLaunchKernelGGL(smin::sample_clips_kernel, dim3(cdiv(T, smin::SAMPLE_ROWS), B), dim3(256), 0, (hipStream_t)stream, raw,
                       (const long long*)offsets, spos, mode, T, Din / 4, video_features, nfeats);
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
