// ahv_wave.h -- reductions over the 64 lanes of one wave, included by ahv_device.h (after key_t): every kernel file sees them.
// Two shapes, and a reduction keeps the one it has -- the order of a float sum is part of its result's bytes:
//  - an xor butterfly (__shfl_xor at 32, 16, .., 1: six ds_bpermute round trips), the result in every lane: wave_max_key,
//    wave_sum_int, wave_max_int, wave_max_f64.  For the one-off reduction at the end of a kernel.
//  - a DPP chain of six row operations, no LDS round trip, for loops that have the reduction on their critical path:
//
//        step  control  meaning        row mask, bank mask of a SUM    row mask of a MAX (bank mask 0xF)
//        1     0x111    row_shr:1      0xF, 0xF                        0xF
//        2     0x112    row_shr:2      0xF, 0xF                        0xF
//        3     0x114    row_shr:4      0xF, 0xE                        0xF
//        4     0x118    row_shr:8      0xF, 0xC                        0xF    -> lane 15 of each row holds its row
//        5     0x142    row_bcast:15   0xA, 0xF                        0xA
//        6     0x143    row_bcast:31   0xC, 0xF                        0xC    -> lane 63 holds the wave
//
//    A sum masks the lanes a step must not reach and reads 0 for a lane without a source (bound_ctrl); its result is valid
//    in lane 63 only.  A max lets a lane that a step does not reach keep its own value (old = the value itself), and is
//    handed to every lane by a readlane of lane 63.
// The open-coded reductions of the encoder, the trilinear kernels, the tracker and the split scorer are not these.
#pragma once

namespace ahv {

__device__ __forceinline__ key_t wave_max_key(key_t k)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const key_t o = __shfl_xor(k, s, 64);
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ int wave_sum_int(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__device__ __forceinline__ int wave_max_int(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(x, off, 64);
        x = o > x ? o : x;
    }
    return x;
}

// (a NaN among the inputs is dropped: the callers reduce scores that are finite or -inf)
__device__ __forceinline__ double wave_max_f64(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(x, off, 64);
        x = o > x ? o : x;
    }
    return x;
}

// wave_max_key by the DPP chain, for the knock-out rounds of the top-K kernels (one reduction per round, K rounds in a row).
// The key is reduced as its two halves: a signed 32-bit max of the score words (one DPP-modified v_max per step), then
// the index word of the lane that holds that score -- read straight from it when it is the only one, else an unsigned max
// over the tied lanes (lowest index = largest word).  A 64-bit compare-and-select per step cost three times as much.
// Every lane gets the result.
template <int kCtrl, int kRows>
__device__ __forceinline__ int max_i32_dpp_step(int x)
{
    const int o = __builtin_amdgcn_update_dpp(x, x, kCtrl, kRows, 0xF, false);
    return o > x ? o : x;
}

template <int kCtrl, int kRows>
__device__ __forceinline__ unsigned max_u32_dpp_step(unsigned x)
{
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, kCtrl, kRows, 0xF, false);
    return o > x ? o : x;
}

__device__ __forceinline__ key_t wave_max_key_dpp(key_t k)
{
    const int hi = (int)(k >> 32);
    const unsigned lo = (unsigned)((unsigned long long)k & 0xFFFFFFFFull);
    int h = hi;
    h = max_i32_dpp_step<0x111, 0xF>(h);
    h = max_i32_dpp_step<0x112, 0xF>(h);
    h = max_i32_dpp_step<0x114, 0xF>(h);
    h = max_i32_dpp_step<0x118, 0xF>(h);
    h = max_i32_dpp_step<0x142, 0xA>(h);
    h = max_i32_dpp_step<0x143, 0xC>(h);
    const int mh = __builtin_amdgcn_readlane(h, 63);
    const unsigned long long tied = __ballot(hi == mh);
    unsigned ml;
    if (__popcll(tied) == 1) {  // uniform: the usual case, one lane holds the largest score
        ml = (unsigned)__builtin_amdgcn_readlane((int)lo, __ffsll((long long)tied) - 1);
    } else {
        unsigned l = hi == mh ? lo : 0u;
        l = max_u32_dpp_step<0x111, 0xF>(l);
        l = max_u32_dpp_step<0x112, 0xF>(l);
        l = max_u32_dpp_step<0x114, 0xF>(l);
        l = max_u32_dpp_step<0x118, 0xF>(l);
        l = max_u32_dpp_step<0x142, 0xA>(l);
        l = max_u32_dpp_step<0x143, 0xC>(l);
        ml = (unsigned)__builtin_amdgcn_readlane((int)l, 63);
    }
    return (key_t)(((unsigned long long)(unsigned)mh << 32) | (unsigned long long)ml);
}

template <int kCtrl, int kRows>
__device__ __forceinline__ float max_f32_dpp_step(float x)
{
    const int xi = __builtin_bit_cast(int, x);
    const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, kCtrl, kRows, 0xF, false));
    return o > x ? o : x;
}

// the wave's largest value (no NaN among the inputs: they are finite scores or -inf), in every lane
__device__ __forceinline__ float wave_max_f32_dpp(float x)
{
    x = max_f32_dpp_step<0x111, 0xF>(x);
    x = max_f32_dpp_step<0x112, 0xF>(x);
    x = max_f32_dpp_step<0x114, 0xF>(x);
    x = max_f32_dpp_step<0x118, 0xF>(x);
    x = max_f32_dpp_step<0x142, 0xA>(x);
    x = max_f32_dpp_step<0x143, 0xC>(x);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// the sum in fp32; valid in lane 63
__device__ __forceinline__ float wave_sum_dpp(float x)
{
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x111, 0xF, 0xF, true));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x112, 0xF, 0xF, true));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x114, 0xF, 0xE, true));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x118, 0xF, 0xC, true));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x142, 0xA, 0xF, true));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x143, 0xC, 0xF, true));
    return x;
}

template <int kCtrl, int kRows, int kBanks>
__device__ __forceinline__ double sum_f64_dpp_step(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kCtrl, kRows, kBanks, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kCtrl, kRows, kBanks, true);
    return x + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the sum in the order of wave_sum_dpp, in fp64 (each half of the double moves by its own DPP); valid in lane 63
__device__ __forceinline__ double wave_sum_dpp_f64(double x)
{
    x = sum_f64_dpp_step<0x111, 0xF, 0xF>(x);
    x = sum_f64_dpp_step<0x112, 0xF, 0xF>(x);
    x = sum_f64_dpp_step<0x114, 0xF, 0xE>(x);
    x = sum_f64_dpp_step<0x118, 0xF, 0xC>(x);
    x = sum_f64_dpp_step<0x142, 0xA, 0xF>(x);
    x = sum_f64_dpp_step<0x143, 0xC, 0xF>(x);
    return x;
}

}  // namespace ahv
