// Compact video banks: fv [V][T][D] held as bf16 or as int8 codes with one fp32 scale per frame, and searched
// without being expanded.  fv enters the model in two places -- the pairs' gate product (smin_pair_assemble) and the first-stage
// contraction (smin_prefilter_scores) --, and in both the decoder is ONE fp32 multiplication (none for bf16) in front of the
// arithmetic the fp32 kernels already do, so a compact bank gives the bits of an fp32 bank holding the decoded values.
//   smin_bank_encode            fv -> codes (and scales): one wave per row of D values;
//   smin_bank_decode            the decoder alone (VideoBank.dequantized, the tests);
//   smin_pair_assemble_compact  smin_pair_assemble over codes: decode, then the gate product; the gathers move bits.
// The first-stage contraction over codes is smin_prefilter_scores_compact (prefilter.hip, through gemm.h's CodeMatQ / PlainMatH), the
// survivors' copy smin_survivors_admit_compact (prefilter_fold.hip).
// The code (smin_hip.h, SMIN_BANK_*): bf16 = round to nearest even of the upper half, NaN -> 0x7fc0; int8 = per row scale = amax / 127
// and q = clamp(rint(x / scale), -127, 127), both divisions correctly rounded (__fdiv_rn: v_div_scale / v_div_fmas / v_div_fixup, never
// a reciprocal approximation), a zero row -> scale 0, a row with a NaN or an infinity -> scale NaN, codes 0 in both cases.
// No atomics, plain stores, no host read, every output element written, every index clamped before it forms an address.
#include "common.h"
#include "gemm.h"
#include "smin_hip.h"

namespace smin {
namespace {

constexpr int BT = 256;                      // threads of a workgroup: four waves, one row each in the encoder

__device__ __forceinline__ unsigned bf16_rne(float x)
{
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;         // a NaN stays a (quiet) NaN: the rounding add could carry it to an infinity
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ bool finite4(float4 x)
{
    const float inf = __uint_as_float(0x7f800000u);
    return fabsf(x.x) < inf && fabsf(x.y) < inf && fabsf(x.z) < inf && fabsf(x.w) < inf;   // (false for a NaN as well)
}
__device__ __forceinline__ unsigned q8(float x, float scale)
{
    const float r = fminf(fmaxf(rintf(__fdiv_rn(x, scale)), -127.0f), 127.0f);
    return (unsigned)(int)r & 0xffu;
}

// One wave per row; lane l owns the quads l, l + 64, ...  int8: pass 1 the row's amax (fmaxf drops a NaN, so non-finite values are
// detected explicitly and voted over the wave), pass 2 the codes (the row is read again: it is in cache).
template <int MODE>
__global__ __launch_bounds__(BT)
void bank_encode_kernel(const float* __restrict__ fv, long long R, int D4, void* __restrict__ codes, float* __restrict__ scale)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
    if (row >= R) return;                                         // (whole waves leave: the votes below are among the lanes of one row)
    const float* x = fv + (size_t)row * D4 * 4;
    if (MODE == SMIN_BANK_BF16) {
        uint2* o = reinterpret_cast<uint2*>(codes) + (size_t)row * D4;
        for (int q = lane; q < D4; q += 64) {
            const float4 v = ldg4(x + 4 * q);
            o[q] = make_uint2(bf16_rne(v.x) | (bf16_rne(v.y) << 16), bf16_rne(v.z) | (bf16_rne(v.w) << 16));
        }
        return;
    }
    float amax = 0.f;
    bool ok = true;
    for (int q = lane; q < D4; q += 64) {
        const float4 v = ldg4(x + 4 * q);
        ok = ok && finite4(v);
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    ok = __all(ok);
    const float s = ok ? __fdiv_rn(amax, 127.0f) : __uint_as_float(0x7fc00000u);
    const bool live = ok && s > 0.f;
    if (lane == 0) scale[row] = s;
    unsigned* o = reinterpret_cast<unsigned*>(codes) + (size_t)row * D4;
    for (int q = lane; q < D4; q += 64) {
        const float4 v = ldg4(x + 4 * q);
        o[q] = live ? q8(v.x, s) | (q8(v.y, s) << 8) | (q8(v.z, s) << 16) | (q8(v.w, s) << 24) : 0u;
    }
}

// four decoded values of row `row`, quad q (the decoder: dec4_q8 / ldg4_bf16 of gemm.h)
template <int MODE>
__device__ __forceinline__ float4 decode_quad(const void* __restrict__ codes, const float* __restrict__ scale, size_t row, int D4, int q)
{
    if (MODE == SMIN_BANK_BF16) return ldg4_bf16(reinterpret_cast<const unsigned short*>(codes) + (row * D4 + q) * 4);
    return dec4_q8(reinterpret_cast<const unsigned*>(codes)[row * D4 + q], scale[row]);
}

template <int MODE>
__global__ __launch_bounds__(BT)
void bank_decode_kernel(const void* __restrict__ codes, const float* __restrict__ scale, int D4, size_t total, float* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * BT + threadIdx.x;
    if (idx >= total) return;
    stg4(out + idx * 4, decode_quad<MODE>(codes, scale, idx / D4, D4, (int)(idx % D4)));
}

// pair_assemble_kernel (corpus.hip) over codes.  One thread per piece of W quads of the P * (T + Nq + 1) output rows: row r of pair p is
// frame r of f (r < T), word r - T of f_w (r < T + Nq) or f_s.  W = 4 (D % 16 == 0): a frame's piece is one 16-byte load of int8 codes
// (two of bf16) and leaves as four float4; W = 1 is the narrow path for any D % 4 == 0.  f = (code * scale) * fs: the decoder's
// multiplication, then video_enc_gate_kernel's; the gathers move bits.  Both indices are clamped before they form an address.
template <int MODE, int W>
__global__ __launch_bounds__(BT)
void pair_assemble_compact_kernel(const void* __restrict__ codes, const float* __restrict__ scale, const float* __restrict__ fs_bank,
                                  const float* __restrict__ fw_bank, const int* __restrict__ video_index, const int* __restrict__ query_index,
                                  int V, int Q, int T, int Nq, int D4, size_t total, float* __restrict__ f, float* __restrict__ fw,
                                  float* __restrict__ fs)
{
    const size_t idx = (size_t)blockIdx.x * BT + threadIdx.x;
    if (idx >= total) return;
    const int DW = D4 / W, R = T + Nq + 1;
    const int d4 = (int)(idx % DW) * W;
    const size_t pr = idx / DW;
    const size_t p = pr / R;
    const int r = (int)(pr - p * R);
    const size_t q = (size_t)min(max(query_index[p], 0), Q - 1);
    float4 s[W];
#pragma unroll
    for (int k = 0; k < W; ++k) s[k] = ldg4(fs_bank + (q * D4 + d4 + k) * 4);
    if (r < T) {
        const size_t v = (size_t)min(max(video_index[p], 0), V - 1);
        const size_t row = v * T + r;
        float4 x[W];
        if (W == 1) {
            x[0] = decode_quad<MODE>(codes, scale, row, D4, d4);
        } else if (MODE == SMIN_BANK_INT8) {
            const uint4 c = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned*>(codes) + row * D4 + d4);
            const float sc = scale[row];
            x[0] = dec4_q8(c.x, sc); x[1 % W] = dec4_q8(c.y, sc); x[2 % W] = dec4_q8(c.z, sc); x[3 % W] = dec4_q8(c.w, sc);
        } else {
            const uint4* c = reinterpret_cast<const uint4*>(reinterpret_cast<const uint2*>(codes) + row * D4 + d4);
            const uint4 a = c[0], b = c[1];
            x[0] = make_float4(__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xffff0000u), __uint_as_float(a.y << 16), __uint_as_float(a.y & 0xffff0000u));
            x[1 % W] = make_float4(__uint_as_float(a.z << 16), __uint_as_float(a.z & 0xffff0000u), __uint_as_float(a.w << 16), __uint_as_float(a.w & 0xffff0000u));
            x[2 % W] = make_float4(__uint_as_float(b.x << 16), __uint_as_float(b.x & 0xffff0000u), __uint_as_float(b.y << 16), __uint_as_float(b.y & 0xffff0000u));
            x[3 % W] = make_float4(__uint_as_float(b.z << 16), __uint_as_float(b.z & 0xffff0000u), __uint_as_float(b.w << 16), __uint_as_float(b.w & 0xffff0000u));
        }
        float* o = f + ((p * T + r) * D4 + d4) * 4;
#pragma unroll
        for (int k = 0; k < W; ++k) stg4(o + 4 * k, f4mul(x[k], s[k]));
    } else if (r < T + Nq) {
        const int w = r - T;
        const float* i = fw_bank + ((q * Nq + w) * D4 + d4) * 4;
        float4 x[W];
#pragma unroll
        for (int k = 0; k < W; ++k) x[k] = ldg4(i + 4 * k);
        float* o = fw + ((p * Nq + w) * D4 + d4) * 4;
#pragma unroll
        for (int k = 0; k < W; ++k) stg4(o + 4 * k, x[k]);
    } else {
        float* o = fs + (p * D4 + d4) * 4;
#pragma unroll
        for (int k = 0; k < W; ++k) stg4(o + 4 * k, s[k]);
    }
}

}  // namespace

// what every entry point over a compact bank checks of (codes, scale, mode), codes aligned to `align` bytes (a power of two):
// bank_codec.hip, prefilter.hip, prefilter_fold.hip
bool bank_code_ok(const void* codes, const float* scale, int mode, int align)
{
    if (mode != SMIN_BANK_BF16 && mode != SMIN_BANK_INT8) return false;
    if (codes == nullptr || ((uintptr_t)codes & (uintptr_t)(align - 1)) != 0) return false;
    return mode == SMIN_BANK_INT8 ? scale != nullptr : scale == nullptr;
}

}  // namespace smin

using namespace smin;

extern "C" int smin_bank_encode(void* stream, const float* fv, int64_t R, int D, int mode, void* codes, float* scale)
{
    SMIN_REQUIRE(R >= 1 && D >= 4 && D % 4 == 0 && R <= (1ll << 40) / D);
    SMIN_REQUIRE(fv != nullptr && ((uintptr_t)fv & 15) == 0 && bank_code_ok(codes, scale, mode, bank_quad_bytes(mode)));
    const long long blocks = (R + BT / 64 - 1) / (BT / 64);
    SMIN_REQUIRE(blocks <= 0x7fffffffll);
    if (mode == SMIN_BANK_BF16)
        hipLaunchKernelGGL(bank_encode_kernel<SMIN_BANK_BF16>, dim3((unsigned)blocks), dim3(BT), 0, (hipStream_t)stream, fv, (long long)R, D / 4, codes, scale);
    else
        hipLaunchKernelGGL(bank_encode_kernel<SMIN_BANK_INT8>, dim3((unsigned)blocks), dim3(BT), 0, (hipStream_t)stream, fv, (long long)R, D / 4, codes, scale);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_bank_decode(void* stream, const void* codes, const float* scale, int64_t R, int D, int mode, float* out)
{
    SMIN_REQUIRE(R >= 1 && D >= 4 && D % 4 == 0 && R <= (1ll << 40) / D);
    SMIN_REQUIRE(out != nullptr && ((uintptr_t)out & 15) == 0 && bank_code_ok(codes, scale, mode, bank_quad_bytes(mode)));
    const size_t total = (size_t)R * (D / 4);
    SMIN_REQUIRE((total + BT - 1) / BT <= 0x7fffffffull);
    const dim3 grid((unsigned)((total + BT - 1) / BT));
    if (mode == SMIN_BANK_BF16)
        hipLaunchKernelGGL(bank_decode_kernel<SMIN_BANK_BF16>, grid, dim3(BT), 0, (hipStream_t)stream, codes, scale, D / 4, total, out);
    else
        hipLaunchKernelGGL(bank_decode_kernel<SMIN_BANK_INT8>, grid, dim3(BT), 0, (hipStream_t)stream, codes, scale, D / 4, total, out);
    SMIN_LAUNCH_CHECK();
    return 0;
}

extern "C" int smin_pair_assemble_compact(void* stream, const void* codes, const float* scale, int mode, const float* fs_bank, const float* fw_bank,
                                          const int32_t* video_index, const int32_t* query_index, int P, int V, int Q, int T, int Nq, int D, float* f,
                                          float* fw, float* fs)
{
    SMIN_REQUIRE(D >= 4 && D % 4 == 0 && P >= 1 && V >= 1 && Q >= 1 && T >= 1 && Nq >= 1);
    SMIN_REQUIRE(bank_code_ok(codes, scale, mode, 16) && fs_bank != nullptr && fw_bank != nullptr && video_index != nullptr && query_index != nullptr);
    SMIN_REQUIRE(f != nullptr && fw != nullptr && fs != nullptr);
    const bool wide = D % 16 == 0;
    const size_t total = (size_t)P * ((size_t)T + Nq + 1) * (D / (wide ? 16 : 4));
    SMIN_REQUIRE((total + BT - 1) / BT <= 0x7fffffffull);
    const dim3 grid((unsigned)((total + BT - 1) / BT));
#define SMIN_ASSEMBLE(MODE, W)                                                                                                                  \
    hipLaunchKernelGGL((pair_assemble_compact_kernel<MODE, W>), grid, dim3(BT), 0, (hipStream_t)stream, codes, scale, fs_bank, fw_bank, video_index, \
                       query_index, V, Q, T, Nq, D / 4, total, f, fw, fs)
    if (mode == SMIN_BANK_BF16) {
        if (wide) SMIN_ASSEMBLE(SMIN_BANK_BF16, 4); else SMIN_ASSEMBLE(SMIN_BANK_BF16, 1);
    } else {
        if (wide) SMIN_ASSEMBLE(SMIN_BANK_INT8, 4); else SMIN_ASSEMBLE(SMIN_BANK_INT8, 1);
    }
#undef SMIN_ASSEMBLE
    SMIN_LAUNCH_CHECK();
    return 0;
}
