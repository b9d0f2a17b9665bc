// ahv_tile.h -- the grid rule of the selection family: what the kernels of ahv_select.hip (modes, fold), ahv_views.hip and
// ahv_posterior.hip share and nothing else.  A sample's N hypotheses are cut into tiles of kTopkTile, one workgroup of
// kTopkThreads per tile and sample, at most kTileGridMax workgroups per sample (a workgroup then walks the tiles x, x + gridDim.x,
// ...); a lane holds four consecutive hypotheses.  Here: the constants, the loaders that state the alignment and ragged-end
// rules once, the workgroup's key reduction, and the host's grid.  Not here: anything a single family owns (the list
// machinery of the top-K kernels, the view weights, the posterior's records).
#pragma once
#include "ahv_device.h"

namespace ahv {

constexpr int kTopkThreads = 256;
constexpr int kTopkPerLane = 4;
constexpr int kTopkTile = kTopkThreads * kTopkPerLane;  // 1024 scores per tile
constexpr int kTileGridMax = 1024;                      // workgroups per sample

// the launch grid of a kernel on this rule: (min(tiles, kTileGridMax), B)
inline dim3 tile_grid(int64_t N, int B)
{
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    return dim3((unsigned)(tiles < kTileGridMax ? tiles : kTileGridMax), (unsigned)B);
}

// ---------------------------------------------------------------------------------
// A lane's four consecutive hypotheses n0 .. n0 + 3 (grid rule of topk_modes_kernel and posterior_partial_kernel: tiles of
// kTopkTile hypotheses, 256 threads, tile t starts at hypothesis t * kTopkTile, n0 = t * kTopkTile + 4 tid).
//  - alignment rule: 16-byte loads only where THAT ADDRESS is 16-byte aligned.  A sample's score row starts at s + b N and a
//    per-sample R row at R + 9 b N: with N % 4 != 0 they start mid-vector, so the tile index says nothing about alignment.
//  - ragged-end rule: a lane whose four hypotheses do not all exist (n0 + 3 >= N) goes element by element and reads no slot
//    at or past N.
// (topk_kernel<true> does not load through these: it shifts its tiles onto the row's 16-byte grid by a, so its lanes straddle
// the row's start as well as its end and its vector test is on n0, not on the address.)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// sc[e] = s[n0 + e], fill where hypothesis n0 + e does not exist
__device__ __forceinline__ void load_scores4(const float* __restrict__ s, long n0, long N, float fill, float (&sc)[4])
{
    if (n0 + 3 < N && aligned16(s + n0)) {
        const float4 q = *reinterpret_cast<const float4*>(s + n0);
        sc[0] = q.x; sc[1] = q.y; sc[2] = q.z; sc[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[e] = n0 + e < N ? s[n0 + e] : fill;
    }
}

// r[e] = the matrix of hypothesis n0 + e (Rb: the sample's row of R).  The four matrices are 144 contiguous bytes: nine
// 16-byte loads for all four, whatever want says; element by element only the matrices that exist and are wanted are read,
// the others come back zero.
__device__ __forceinline__ void load_rotations4(const float* __restrict__ Rb, long n0, long N, const bool (&want)[4],
                                                float (&r)[4][9])
{
    const float* rp = Rb + n0 * 9;
    if (n0 + 3 < N && aligned16(rp)) {
        float4 q[9];
#pragma unroll
        for (int v = 0; v < 9; ++v) q[v] = reinterpret_cast<const float4*>(rp)[v];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int f = e * 9 + i;
                const float4 v = q[f >> 2];
                r[e][i] = (f & 3) == 0 ? v.x : (f & 3) == 1 ? v.y : (f & 3) == 2 ? v.z : v.w;
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 9; ++i) r[e][i] = (n0 + e < N && want[e]) ? rp[e * 9 + i] : 0.0f;
    }
}

// sl[e] = slot[n0 + e], fill where hypothesis n0 + e does not exist (load_scores4's rules)
__device__ __forceinline__ void load_slots4(const int* __restrict__ s, long n0, long N, int fill, int (&sl)[4])
{
    if (n0 + 3 < N && aligned16(s + n0)) {
        const int4 q = *reinterpret_cast<const int4*>(s + n0);
        sl[0] = q.x; sl[1] = q.y; sl[2] = q.z; sl[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) sl[e] = n0 + e < N ? s[n0 + e] : fill;
    }
}

typedef long long i64x2 __attribute__((ext_vector_type(2)));  // two packed keys: one 16-byte access

// the workgroup's largest key -> one atomicMax into *dst (skipped when nothing survives: *dst was filled kKeyEmpty).  wl: one
// LDS word per wave.  The modes kernels reduce their survivors through it, the fuse kernels of ahv_views.hip their fused keys.
__device__ __forceinline__ void modes_publish(key_t best, key_t* wl, key_t* dst)
{
    const key_t m = wave_max_key_dpp(best);
    if ((threadIdx.x & 63) == 0) wl[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        key_t r = wl[0];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) r = wl[w] > r ? wl[w] : r;
        if (r != kKeyEmpty) atomicMax(dst, r);
    }
}

}  // namespace ahv
