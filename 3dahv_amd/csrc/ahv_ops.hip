// ahv_ops.hip -- op-level drop-in kernels: each materialises the tensor the
// reference's corresponding call returns, so the reference's own call sequence
// (rotate_volume -> forward_3d2d -> mul/sum/mean -> max) runs unchanged on HIP.
// These are the HBM-bound siblings of the fused scorer (ahv_score.hip).
#include "ahv_device.h"
#include "ahv_dual.h"
#include "ahv_exact.h"

namespace ahv {

// ---------------------------------------------------------------------------------
// rotate_volume, fast path: volume (16,8,8,8) shared by all N hypotheses (the stride-0
// expand of test_co3d.py:137).  HBM: 36 B in + 32 KiB out per hypothesis -> write-bandwidth bound,
// provided the kernel needs less than the ~3 500 cycles per hypothesis and CU that 5.7 TB/s leave it.
// Rounds 1-4 (tri_coef + tri_blend per voxel) needed ~2 100 vector instructions per hypothesis and reached 5.14 TB/s.
// Round 5: the fused scorer's gather -- hat weights on a clamped base row, one base address per voxel, the request ring,
// packed FMAs, the point-mirror quarters (ahv_dual.h: ~900 vector instructions per hypothesis) -- with a store that goes
// straight to global memory: one non-temporal 4-byte store per channel and pass, two whole 128-byte lines per instruction.
// No LDS besides the source image (47.5 KiB) -> three workgroups = 12 waves per CU at <= 168 registers (ring depth 2:
// 3 and 4 rows spill).  First built with a per-wave LDS image and 16-byte stores (8 waves per CU): 1.245 ms against
// 1.19-1.21 ms for this one on the same box, N = 200 000 (5.27 vs 5.43-5.52 TB/s; the minimum of ten launches 5.8).
// What bounds it is the store stream itself: the same kernel with the gather removed and tools/store_probe.cpp (this store
// pattern, others, and a plain fill, from the same persistent grid) write 6.55 GB at 5.3-6.1 TB/s whatever the pattern --
// one 32 KiB region per wave, ~3 000 regions open at once -- and the gather with its bank conflicts switched off is no
// faster (diagnostic builds of round 5, HISTORY.md; their code was last in commit 86a1f1c).
// A NaN / inf voxel: the workgroup sees it while staging and every hypothesis of the launch goes through
// exact_gather_quarter_global (ahv_exact.h: grid_sample's per-corner zeros padding, utils.py:129) instead.
// ---------------------------------------------------------------------------------
constexpr int kRotThreads = 256;
constexpr int kRotDepth = 2;  // rows the gather requests ahead: 2 -> 160 registers, 3 / 4 -> 8 / 22 spills and slower

// Where a blended voxel goes: straight to out[n][c][...], one non-temporal 4-byte store per channel.  In a pass the 64 lanes
// own the voxels (a0, 4 p + bq, e) of the quarter -- two runs of 32 consecutive floats per channel plane -- so every store
// instruction writes two whole 128-byte lines.
struct RotStoreGlobal {
    static constexpr bool kXdlKernel = kFp32LowHalf;
    static constexpr int kDepth = kRotDepth;
    float* d[2];  // the lane's voxel of pass 0 / pass 1 in channel plane 0 of this quarter
    __device__ __forceinline__ void operator()(int p, const f32x2 (&o)[8]) const
    {
        float* dst = d[p];
#pragma unroll
        for (int c = 0; c < 16; ++c) __builtin_nontemporal_store(o[c >> 1][c & 1], dst + c * 512);
    }
};

template <bool MIR>
__device__ __forceinline__ void rot_quarter(HatState& st, float* oq, const GatherDst& dst)
{
    f32x2 o[8];
    const RotStoreGlobal store = {{oq + (MIR ? dst.m0 : dst.o0), oq + (MIR ? dst.m1 : dst.o1)}};
    HatSteps<0, RotStoreGlobal, MIR>::run(st, o, store);
}

__global__ __launch_bounds__(kRotThreads, 3) void rotate_volume_16x8_kernel(
    const float* __restrict__ vol, const float* __restrict__ R, long N, float* __restrict__ out)
{
    __shared__ __attribute__((aligned(1024))) float srcT[kSrcFloats];
    __shared__ unsigned nf;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) nf = 0u;
    __syncthreads();
    {
        bool bad = false;
        for (int i = tid; i < 16 * 512; i += kRotThreads) {
            const int c = i >> 9, v = i & 511;
            const float x = vol[i];
            bad = bad || non_finite(x);
            srcT[((v >> 6) * kSrcPlaneRows + ((v >> 3) & 7) * kSrcRowsY + (v & 7)) * kSrcStride + c] = x;
        }
        if (bad) nf = 1u;
    }
    __syncthreads();
    const bool exact = __builtin_amdgcn_readfirstlane((int)nf) != 0;
    const GatherLane glane = gather_lane(lane);
    GatherDst gdst = gather_dst_linear(lane);
    asm volatile("" : "+v"(gdst.m0), "+v"(gdst.m1));
    const int rl = lane < 9 ? lane : 8;
    const long nstep = (long)gridDim.x * 4;
    long n = (long)blockIdx.x * 4 + wave;
    float Rn = n < N ? R[n * 9 + rl] : 0.0f;
    for (; n < N; n += nstep) {
        float Rm[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rm[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Rn), i));
        Rn = R[(n + nstep < N ? n + nstep : n) * 9 + rl];
        float* o = out + n * (16 * 512);
        if (!exact) {
            GatherHyp gh;
            gather_hyp(gh, Rm, glane);
            HatState st;
            // quarters in the order 0, 3, 1, 2: quarter 3 - Q is the point mirror of quarter Q and reuses its set-up
            hat_prologue<0, kFp32LowHalf, kRotDepth>(st, srcT, gh);
            rot_quarter<false>(st, o, gdst);
            hat_prologue_mirror<kRotDepth>(st, srcT);
            rot_quarter<true>(st, o + 3 * 128, gdst);
            hat_prologue<1, kFp32LowHalf, kRotDepth>(st, srcT, gh);
            rot_quarter<false>(st, o + 128, gdst);
            hat_prologue_mirror<kRotDepth>(st, srcT);
            rot_quarter<true>(st, o + 2 * 128, gdst);
        } else {
            // a NaN / inf voxel: every hypothesis corner by corner as grid_sample does it (ahv_exact.h), through the
            // same lane -> voxel map as the stores above expect nothing of: each lane writes its own voxels
#pragma unroll 1
            for (int q = 0; q < 4; ++q) exact_gather_quarter_global(o + q * 128, srcT, Rm, q, lane);
        }
    }
}

// ---------------------------------------------------------------------------------
// rotate_volume, generic path: any C, D, H, W and any batch stride (utils.py:113-131
// accepts every 5-D volume).  One thread per output voxel, channels looped; the source
// is read through the caches.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void axis_generic(float g, int size, float& w0, float& w1, long& i0, long& i1, bool& in0, bool& in1)
{
    float i = ((g + 1.0f) * (float)size - 1.0f) * 0.5f;
    i = fminf(fmaxf(i, -2.0f), (float)size + 1.0f);
    const float fl = floorf(i);
    const float t = i - fl;
    const int a = (int)fl, b = a + 1;
    in0 = a >= 0 && a < size;
    in1 = b >= 0 && b < size;
    w0 = in0 ? 1.0f - t : 0.0f;
    w1 = in1 ? t : 0.0f;
    i0 = min(max(a, 0), size - 1);
    i1 = min(max(b, 0), size - 1);
}

__global__ __launch_bounds__(256) void rotate_volume_generic_kernel(
    const float* __restrict__ vol, long vol_batch_stride, const float* __restrict__ R, long N, int C, int D,
    int H, int W, float* __restrict__ out)
{
    const long plane = (long)D * H * W;
    const long total = N * plane;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / plane;
        const long v = i - n * plane;
        const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((long)W * H));
        const float* r = R + n * 9;
        const float x = (2.0f * w + 1.0f) / (float)W - 1.0f;
        const float y = (2.0f * h + 1.0f) / (float)H - 1.0f;
        const float z = (2.0f * d + 1.0f) / (float)D - 1.0f;
        const float gx = r[0] * x + r[1] * y + r[2] * z;
        const float gy = r[3] * x + r[4] * y + r[5] * z;
        const float gz = r[6] * x + r[7] * y + r[8] * z;
        float wx[2], wy[2], wz[2];
        long ox[2], oy[2], oz[2];
        bool ix[2], iy[2], iz[2];
        axis_generic(gx, W, wx[0], wx[1], ox[0], ox[1], ix[0], ix[1]);
        axis_generic(gy, H, wy[0], wy[1], oy[0], oy[1], iy[0], iy[1]);
        axis_generic(gz, D, wz[0], wz[1], oz[0], oz[1], iz[0], iz[1]);
        float wgt[8];
        long off[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
            wgt[k] = wz[dz] * wy[dy] * wx[dx];
            // zeros padding is per corner: an out-of-range corner is SKIPPED (its weight here is 0, but 0 * a non-finite
            // voxel would be NaN where F.grid_sample leaves the voxel out); an in-range corner counts even with weight 0
            off[k] = (iz[dz] && iy[dy] && ix[dx]) ? (oz[dz] * H + oy[dy]) * W + ox[dx] : -1;
        }
        const float* src = vol + n * vol_batch_stride;
        float* o = out + n * C * plane + v;
        for (int c = 0; c < C; ++c) {
            const float* sc = src + c * plane;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (off[k] >= 0) acc += wgt[k] * sc[off[k]];
            o[c * plane] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------
// Adjoint of rotate_volume w.r.t. the volume (the reference's rotate_volume is differentiable and
// infoNCE_loss back-propagates through it, modules/model_co3d.py:49-54): every output voxel scatters
// its gradient to the 8 trilinear corners it was blended from, with the forward's weights (zero for
// corners outside the volume).  grad_vol is zeroed by the caller; sums use float atomics, so the
// result is reproducible to rounding, not bitwise.  With vol_batch_stride = 0 (the stride-0 expand
// the reference passes) all N hypotheses accumulate into ONE volume.  Compatibility path for
// unmodified reference scripts; the training path proper is the fused backward (ahv_backward.hip).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rotate_volume_backward_kernel(
    const float* __restrict__ grad_out, long vol_batch_stride, const float* __restrict__ R, long N, int C, int D,
    int H, int W, float* __restrict__ grad_vol)
{
    const long plane = (long)D * H * W;
    const long total = N * plane;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / plane;
        const long v = i - n * plane;
        const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((long)W * H));
        const float* r = R + n * 9;
        const float x = (2.0f * w + 1.0f) / (float)W - 1.0f;
        const float y = (2.0f * h + 1.0f) / (float)H - 1.0f;
        const float z = (2.0f * d + 1.0f) / (float)D - 1.0f;
        const float gx = r[0] * x + r[1] * y + r[2] * z;
        const float gy = r[3] * x + r[4] * y + r[5] * z;
        const float gz = r[6] * x + r[7] * y + r[8] * z;
        float wx[2], wy[2], wz[2];
        long ox[2], oy[2], oz[2];
        bool ix[2], iy[2], iz[2];
        axis_generic(gx, W, wx[0], wx[1], ox[0], ox[1], ix[0], ix[1]);
        axis_generic(gy, H, wy[0], wy[1], oy[0], oy[1], iy[0], iy[1]);
        axis_generic(gz, D, wz[0], wz[1], oz[0], oz[1], iz[0], iz[1]);
        float wgt[8];
        long off[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
            wgt[k] = wz[dz] * wy[dy] * wx[dx];
            off[k] = (oz[dz] * H + oy[dy]) * W + ox[dx];
            if (!(iz[dz] && iy[dy] && ix[dx])) wgt[k] = 0.0f;  // skipped below: an out-of-range corner receives nothing
        }
        float* dst = grad_vol + n * vol_batch_stride;
        const float* g = grad_out + n * C * plane + v;
        for (int c = 0; c < C; ++c) {
            const float go = g[c * plane];
            float* dc = dst + c * plane;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (wgt[k] != 0.0f)
                    __hip_atomic_fetch_add(dc + off[k], wgt[k] * go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------
// forward_3d2d (modules/modules.py:112-124) on materialised volumes [M][16][8][8][8].
// Same wave-per-item MFMA contraction as the fused scorer; the quarter buffers are
// filled from HBM instead of by the trilinear gather.  32 KiB in + 8 KiB out per item.
// ---------------------------------------------------------------------------------
constexpr int kF32Threads = 256;
constexpr int kF32LdsFloats = 4 * 2 * kQuarterFloats;

template <int Q>
__device__ __forceinline__ void stage_quarter(float* buf, const float* __restrict__ vol, int lane)
{
    // quarter Q of channel c = 128 contiguous floats at c*512 + Q*128; a lane moves 2 of them
    const int i = 2 * lane;
    const int a0 = i >> 6, b = (i >> 3) & 7, e = i & 7;
    const int o0 = qoff(a0, b, e), o1 = qoff(a0, b, e + 1);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float2 v = *reinterpret_cast<const float2*>(vol + c * 512 + Q * 128 + i);
        buf[c * 128 + o0] = v.x;
        buf[c * 128 + o1] = v.y;
    }
}

__global__ __launch_bounds__(kF32Threads, 1) void forward_3d2d_kernel(
    const float* __restrict__ vol, const float* __restrict__ W1, const float* __restrict__ W2,
    const float* __restrict__ b2, long M, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* buf0 = smem + wave * (2 * kQuarterFloats);
    float* buf1 = buf0 + kQuarterFloats;
    HeadFrags f;
    load_head_frags(f, W1, W2, b2, lane);
    const int n16 = lane & 15, kq = lane >> 4;
    for (long m = (long)blockIdx.x * 4 + wave; m < M; m += (long)gridDim.x * 4) {
        const float* V = vol + m * (16 * 512);
        f32x4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        stage_quarter<0>(buf0, V, lane);
        stage_quarter<1>(buf1, V, lane);
        wave_lds_fence();
        gemm1_quarter<0>(acc, f, buf0, lane);
        gemm1_quarter<1>(acc, f, buf1, lane);
        wave_lds_fence();
        stage_quarter<2>(buf0, V, lane);
        stage_quarter<3>(buf1, V, lane);
        wave_lds_fence();
        gemm1_quarter<2>(acc, f, buf0, lane);
        gemm1_quarter<3>(acc, f, buf1, lane);
        wave_lds_fence();
        f32x4 v[2][4];
        gemm2(v, acc, f);
        float* o = out + m * (32 * 64);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float ss = 0.0f;
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r) ss += v[m2][t][r] * v[m2][t][r];
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            const float nrm = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize clamp_min(eps)
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[(16 * m2 + 4 * kq + r) * 64 + 16 * t + n16] = v[m2][t][r] / nrm;
        }
    }
}

// ---------------------------------------------------------------------------------
// forward_3d2d, throughput path: the "dual" structure of the fused scorer (ahv_dual.h): 512 threads = two
// waves per SIMD, one item per wave, W1 as an LDS fragment table, one 8-KiB quarter image per wave filled
// straight from HBM (next quarter's loads are in flight while the current one is contracted).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void forward_3d2d_dual_kernel(
    const float* __restrict__ vol, const float* __restrict__ W1, const float* __restrict__ W2,
    const float* __restrict__ b2, long M, float* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float lds_w1[kW1TableFloats];
    __shared__ __attribute__((aligned(16))) float lds_q[8 * kQuarterFloats];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* buf = lds_q + wave * kQuarterFloats;
    stage_w1_table(lds_w1, W1, tid, 512);
    DualFrags f;
    load_dual_frags(f, W2, b2, lane);
    __syncthreads();
    const int n16 = lane & 15, kq = lane >> 4;
    const int i2 = 2 * lane, sa0 = i2 >> 6, sb = (i2 >> 3) & 7, se = i2 & 7;
    const int o0 = qoff(sa0, sb, se), o1 = qoff(sa0, sb, se + 1);
    const long mstep = (long)gridDim.x * 8;
    long m = (long)wave * gridDim.x + blockIdx.x;
    f32x2 cur[16], nxt[16];
    if (m < M) {
#pragma unroll
        for (int c = 0; c < 16; ++c) cur[c] = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(vol + m * (16 * 512) + i2 + c * 512));
    }
    for (; m < M; m += mstep) {
        const float* V = vol + m * (16 * 512) + i2;
        // quarter 3's prefetch is the NEXT item's quarter 0 (the last item re-reads its own): no first-touch wait per item
        const float* Vn = vol + (m + mstep < M ? m + mstep : m) * (16 * 512) + i2;
        f32x4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#define AHV_F3_QUARTER(Q)                                                                                   \
        _Pragma("unroll") for (int c = 0; c < 16; ++c)                                                      \
            nxt[c] = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>((Q < 3 ? V + (Q + 1) * 128 : Vn) + c * 512)); \
        _Pragma("unroll") for (int c = 0; c < 16; ++c) { buf[c * 128 + o0] = cur[c][0]; buf[c * 128 + o1] = cur[c][1]; } \
        wave_lds_fence();                                                                                   \
        gemm1_quarter_pipe<Q>(acc, lds_w1, buf, lane, [] {});                                               \
        wave_lds_fence();                                                                                   \
        _Pragma("unroll") for (int c = 0; c < 16; ++c) cur[c] = nxt[c];
        AHV_F3_QUARTER(0)
        AHV_F3_QUARTER(1)
        AHV_F3_QUARTER(2)
        AHV_F3_QUARTER(3)
#undef AHV_F3_QUARTER
        f32x4 v[2][4];
        gemm2_dual_exact(v, acc, f);  // the op-level drop-in materialises the reference's tensor: F.relu's NaN propagation too
        float* o = out + m * (32 * 64);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float ss = 0.0f;
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r) ss += v[m2][t][r] * v[m2][t][r];
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            // v / max(|v|, eps) as v * (1 / max(|v|, eps)): ONE correctly rounded division per position instead of eight per
            // lane (an IEEE division is ~10 vector instructions, and fp32 MFMAs overlap none of them: 320 of an item's ~900);
            // each feature within 1 ulp of the quotient
            const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[(16 * m2 + 4 * kq + r) * 64 + 16 * t + n16] = v[m2][t][r] * inv;
        }
    }
}

// ---------------------------------------------------------------------------------
// forward_3d2d for a handful of items (the per-pair target feature, test_co3d.py:141): latency matters,
// not throughput.  One 512-thread workgroup per item.  W1 is copied once, coalesced, into LDS with a
// 386-float row stride (the fragment reads W1[row][k0 + kq] of a half-wave then hit 32 different banks); wave
// (q, kh) contracts quarter q with the x slab + half of the z slab (kh = 0) or the y slab + the other half
// (kh = 1); the eight partial accumulators meet in LDS and waves 0-3 each finish one position tile
// (ReLU, GEMM2, bias, normalise).
// ---------------------------------------------------------------------------------
constexpr int kW1PadStride = 386;  // bank = (2 row + k) mod 32: 16 rows x 2 k-groups of a half-wave hit 32 banks

__global__ __launch_bounds__(512) void forward_3d2d_small_kernel(
    const float* __restrict__ vol, const float* __restrict__ W1, const float* __restrict__ W2,
    const float* __restrict__ b2, float* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float qbuf[4][kQuarterFloats];
    __shared__ __attribute__((aligned(16))) float part[8][8][64][4];
    __shared__ float w1s[32 * kW1PadStride];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = wave & 3, kh = wave >> 2;
    const int n = lane & 15, kq = lane >> 4, i0 = n >> 3, j = n & 7, row = lane & 15;
    const float* V = vol + (long)blockIdx.x * (16 * 512);
    for (int i = tid; i < 32 * 96; i += 512) {  // 96 float4 per W1 row
        const int r = i / 96, k4 = i - r * 96;
        const f32x4 w = *reinterpret_cast<const f32x4*>(W1 + r * 384 + 4 * k4);
        float* d = w1s + r * kW1PadStride + 4 * k4;
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
    }
    {   // quarter q of channel c = 128 contiguous floats at c*512 + q*128; the two waves of a quarter take 8 channels each
        float* buf = qbuf[q];
        const int i = 2 * lane, a0 = i >> 6, bb = (i >> 3) & 7, e = i & 7;
        const int o0 = qoff(a0, bb, e), o1 = qoff(a0, bb, e + 1);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            const int c = 8 * kh + cc;
            const float2 v = *reinterpret_cast<const float2*>(V + c * 512 + q * 128 + i);
            buf[c * 128 + o0] = v.x;
            buf[c * 128 + o1] = v.y;
        }
    }
    __syncthreads();
    const float* buf = qbuf[q];
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* w0 = w1s + row * kW1PadStride;
    const float* w1 = w1s + (16 + row) * kW1PadStride;
    // the x / y slab lands in n-tile q; which tile that is must be a compile-time register index
#define AHV_XY(T)                                                                                          \
    _Pragma("unroll") for (int c = 0; c < 16; ++c) _Pragma("unroll") for (int hh = 0; hh < 2; ++hh) {        \
        const int k = 128 * kh + c * 8 + 4 * hh + kq;                                                      \
        const float bv = kh ? buf[c * 128 + qoff(i0, 4 * hh + kq, j)] : buf[c * 128 + qoff(i0, j, 4 * hh + kq)]; \
        acc[0][T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[k], bv, acc[0][T], 0, 0, 0);                    \
        acc[1][T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[k], bv, acc[1][T], 0, 0, 0);                    \
    }
    if (q == 0) { AHV_XY(0) } else if (q == 1) { AHV_XY(1) } else if (q == 2) { AHV_XY(2) } else { AHV_XY(3) }
#undef AHV_XY
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const int cp = 4 * kh + cc;
        const int kz = 256 + (2 * cp + (kq >> 1)) * 8 + 2 * q + (kq & 1);
        const float a0 = w0[kz], a1 = w1[kz];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float bz = buf[(2 * cp + (kq >> 1)) * 128 + qoff(kq & 1, 2 * t + i0, j)];
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bz, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bz, acc[1][t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(part[wave][m * 4 + t][lane]) = acc[m][t];
    __syncthreads();
    if (wave >= 4) return;
    const int t = wave;  // this wave finishes positions 16t .. 16t+15
    f32x4 u[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        u[m] = *reinterpret_cast<const f32x4*>(part[0][m * 4 + t][lane]);
#pragma unroll
        for (int w = 1; w < 8; ++w) u[m] += *reinterpret_cast<const f32x4*>(part[w][m * 4 + t][lane]);
    }
    f32x4 v[2];
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[m2][r] = b2[16 * m2 + 4 * kq + r];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a20 = W2[row * 32 + 16 * m + 4 * kq + r], a21 = W2[(16 + row) * 32 + 16 * m + 4 * kq + r];
            const float x = u[m][r] < 0.0f ? 0.0f : u[m][r];  // F.relu: a NaN stays a NaN (v_max would drop it)
            v[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a20, x, v[0], 0, 0, 0);
            v[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a21, x, v[1], 0, 0, 0);
        }
    float ss = 0.0f;
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss += v[m2][r] * v[m2][r];
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    float* o = out + (long)blockIdx.x * (32 * 64);
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * m2 + 4 * kq + r) * 64 + 16 * t + n] = v[m2][r] / nrm;
}

// ---------------------------------------------------------------------------------
// score (test_co3d.py:143): one wave per (b, n); 8 KiB of f_src streamed per hypothesis.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_features_kernel(const float* __restrict__ f_src,
                                                             const float* __restrict__ f_tgt, int B, long N,
                                                             float* __restrict__ scores)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nw = (long)gridDim.x * 4;
    for (long i = wave; i < (long)B * N; i += nw) {
        const long b = i / N;
        const f32x4* s = reinterpret_cast<const f32x4*>(f_src + i * 2048);
        const f32x4* t = reinterpret_cast<const f32x4*>(f_tgt + b * 2048);
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const f32x4 a = __builtin_nontemporal_load(s + k * 64 + lane);
            const f32x4 c = t[k * 64 + lane];
            acc += a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3];
        }
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) acc += __shfl_xor(acc, sft, 64);
        if (lane == 0) scores[i] = acc * (1.0f / 64.0f);
    }
}

// ---------------------------------------------------------------------------------
// arg-max over materialised scores (test_co3d.py:145), same packed key as the fused path.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ scores, int B, long N,
                                                     long n_offset, key_t* __restrict__ best_key)
{
    const int b = blockIdx.y;
    const float* s = scores + (long)b * N;
    key_t best = kKeyEmpty;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
        const key_t k = pack_key(s[n], (unsigned)(n_offset + n));
        best = k > best ? k : best;
    }
    best = wave_max_key(best);
    if ((threadIdx.x & 63) == 0 && best != kKeyEmpty) atomicMax(best_key + b, best);
}

// ---------------------------------------------------------------------------------
// Coarse-to-fine support (BASELINE.json configs[4]; build-defined, the reference scores one flat
// set): refinement hypotheses R_fine[b][n] = R[idx_b] * D[n], where idx_b is decoded on the device from
// the packed key of the coarse stage and D is a fixed set of small rotations.  Graph-capturable.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compose_rotations_kernel(const key_t* __restrict__ best_key,
                                                                const float* __restrict__ R, long r_batch_stride,
                                                                long n_offset, long N, const float* __restrict__ D,
                                                                long N2, int B, float* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * N2) return;
    const int b = (int)(i / N2);
    const long n = i - (long)b * N2;
    const key_t key = best_key[b];
    long idx = key_index(key) - n_offset;
    idx = (key == kKeyEmpty || idx < 0 || idx >= N) ? 0 : idx;  // nothing scored / foreign shard: stay in bounds
    const float* r = R + (long)b * r_batch_stride + idx * 9;
    const float* d = D + n * 9;
    float* o = out + i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = r[a * 3] * d[c] + r[a * 3 + 1] * d[3 + c] + r[a * 3 + 2] * d[6 + c];
}

// unpack + gather in one launch: (best score, global index, R_pred = R[idx]) of test_co3d.py:145-146.
// reset: the key is handed back EMPTY, ready for the next verify step's atomic max (the step then needs no launch
// of its own to clear it: stream order puts this kernel between the two scorers).
__global__ void select_rotation_kernel(key_t* __restrict__ best_key, const float* __restrict__ R, long r_batch_stride,
                                       long n_offset, long N, int B, float* __restrict__ R_out,
                                       float* __restrict__ best_score, long* __restrict__ best_idx, bool reset)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const key_t k = best_key[b];
    if (reset) best_key[b] = kKeyEmpty;
    const long gidx = (k == kKeyEmpty) ? -1l : key_index(k);
    if (best_score) best_score[b] = (k == kKeyEmpty) ? -INFINITY : key_score(k);
    if (best_idx) best_idx[b] = gidx;
    if (R_out) {
        const long loc = gidx - n_offset;
        const bool mine = (k != kKeyEmpty) && loc >= 0 && loc < N;  // with sharding only the owner rank holds the row
        const float* r = R + (long)b * r_batch_stride + (mine ? loc : 0) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) R_out[b * 9 + e] = mine ? r[e] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------
// K best hypotheses (the list counterpart of argmax_kernel / select_rotation_kernel / compose_rotations_kernel).
// A list is K packed keys in descending SIGNED order, distinct, padded with kKeyEmpty.  With pack_key as it is that order
// is torch.sort(scores, dim=1, descending=True, stable=True) truncated to K (NaN first, lowest index among equal
// scores, -0 = +0); it is NOT torch.topk's order, which leaves ties unspecified.
//
// Everything on the critical path stays inside ONE wave: no barrier and no LDS round trip per round.
//  - scores -> lists (topk_kernel<true>): a workgroup of four waves walks tiles of kTopkTile scores; a lane holds four
//    candidates (one 16-byte load), and each wave on its own runs K knock-out rounds over its 256 -- a wave-wide max by DPP
//    row operations, the lane that offered the winner moves to its largest key strictly below it -- and leaves a sorted
//    K-list in LDS.  The four wave lists and the workgroup's running list are then merged by counting ranks (a fresh
//    list: all keys distinct) or, when the caller's list is merged into in the same launch, by their HEADS.
//  - lists -> list (merge_heads): one lane per sorted list; a round is the wave-wide max of the heads, and every lane
//    whose head is the winner steps to its next entry (so a key met in several lists is taken once).  Up to 63 lists and
//    the running list per pass; more lists are taken in passes.  This is ahv_topk_merge_keys, and the second launch of
//    ahv_topk_f32.
// Order, distinctness and the tie rule fall out of the integer compare.  A sample's N scores are spread over up to
// kTopkMaxParts workgroups whose lists go to the workspace; the second launch merges them into the caller's list ACROSS A
// KERNEL BOUNDARY -- no ticket, no loads that must dodge a stale per-XCD L2 line.  N <= one tile: one launch, straight into
// the list.  (The first version ran every round workgroup-wide -- eight candidates per lane, four LDS words and a barrier
// per round, in both launches: 1.1 us per round and pair of launches, slower than torch.topk + gather at K = 64.)
// ---------------------------------------------------------------------------------
constexpr int kTopkThreads = 256;
constexpr int kTopkPerLane = 4;
constexpr int kTopkTile = kTopkThreads * kTopkPerLane;  // 1024 scores per tile
constexpr int kTopkMaxParts = 63;                       // partial lists per sample: with the running list, one lane each
constexpr int kTopkMaxK = 64;

// wave 0 only: merge sorted lists by their heads into out[0..K) (LDS).  mine: this lane's list (K keys, descending), or
// nullptr for a lane without one.
__device__ __forceinline__ void merge_heads(const key_t* mine, int K, key_t* out)
{
    const int lane = threadIdx.x & 63;
    int pos = 0;
    key_t head = mine ? mine[0] : kKeyEmpty;
    for (int r = 0; r < K; ++r) {
        const key_t m = wave_max_key_dpp(head);
        if (lane == 0) out[r] = m;
        if (m == kKeyEmpty) {  // fewer than K distinct keys: pad (uniform over the wave)
            for (int j = r + 1 + lane; j < K; j += 64) out[j] = kKeyEmpty;
            break;
        }
        while (head >= m) {  // my head won (or repeats the winner): step past it; kKeyEmpty < m ends the walk
            ++pos;
            head = pos < K ? mine[pos] : kKeyEmpty;
        }
    }
}

// one wave, K knock-out rounds over the lanes' candidates c[0..kTopkPerLane): out[0..K) (LDS) = the wave's sorted list
__device__ __forceinline__ void wave_knock_out(const key_t (&c)[kTopkPerLane], int K, key_t* out)
{
    const int lane = threadIdx.x & 63;
    key_t mine = c[0];
#pragma unroll
    for (int i = 1; i < kTopkPerLane; ++i) mine = c[i] > mine ? c[i] : mine;
    for (int r = 0; r < K; ++r) {
        const key_t m = wave_max_key_dpp(mine);
        if (lane == 0) out[r] = m;
        if (m == kKeyEmpty) {
            for (int j = r + 1 + lane; j < K; j += 64) out[j] = kKeyEmpty;
            break;
        }
        if (mine == m) {  // knocked out: my largest key strictly below the winner
            key_t nxt = kKeyEmpty;
#pragma unroll
            for (int i = 0; i < kTopkPerLane; ++i) nxt = (c[i] < m && c[i] > nxt) ? c[i] : nxt;
            mine = nxt;
        }
    }
}

// kScores: src = scores [B][N] (+ n_offset); workgroup (x, b) takes the tiles x, x + gridDim.x, ... of sample b.  Tiles are
// laid on the 16-byte grid of the sample's row (a = the row's misalignment in floats), so that a lane's four scores are
// one 16-byte load wherever all four exist; the ragged ends go element by element.
// !kScores: src = lists [N][B][K] (N lists per sample), every one sorted as a list is.
// carry: the list starts as out[b][0..K) (merge into) instead of empty.  out: [gridDim.x][B][K].
template <bool kScores>
__global__ __launch_bounds__(kTopkThreads) void topk_kernel(const void* __restrict__ src, int B, long N, long n_offset, int K,
                                                            key_t* __restrict__ out, bool carry)
{
    __shared__ key_t run[2][kTopkMaxK];  // the running list and the one being built
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    key_t* dst = out + ((long)blockIdx.x * B + b) * K;
    if (tid < K) run[0][tid] = carry ? dst[tid] : kKeyEmpty;
    int cur = 0;
    if constexpr (kScores) {
        __shared__ key_t wl[4][kTopkMaxK];  // the four wave lists of a tile
        const float* s = static_cast<const float*>(src) + (long)b * N;
        const long a = (long)((reinterpret_cast<unsigned long long>(s) >> 2) & 3ull);
        const long tiles = (N + a + kTopkTile - 1) / kTopkTile;
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            key_t c[kTopkPerLane];
            const long n0 = t * kTopkTile + (long)tid * 4 - a;  // first of the lane's four scores
            if (n0 >= 0 && n0 + 3 < N) {
                const float4 q = *reinterpret_cast<const float4*>(s + n0);
                c[0] = pack_key(q.x, (unsigned)(n_offset + n0));
                c[1] = pack_key(q.y, (unsigned)(n_offset + n0 + 1));
                c[2] = pack_key(q.z, (unsigned)(n_offset + n0 + 2));
                c[3] = pack_key(q.w, (unsigned)(n_offset + n0 + 3));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long n = n0 + e;
                    c[e] = (n >= 0 && n < N) ? pack_key(s[n], (unsigned)(n_offset + n)) : kKeyEmpty;
                }
            }
            wave_knock_out(c, K, wl[wave]);
            __syncthreads();  // the four wave lists (and, first time round, run[0]) are in LDS
            if (carry) {
                if (wave == 0) merge_heads(lane < 4 ? wl[lane] : lane == 4 ? run[cur] : nullptr, K, run[cur ^ 1]);
            } else {
                // A fresh list: the five lists hold keys of different hypotheses, all distinct, so a key's place in the
                // merged list is the number of keys above it -- counted by all 256 lanes at once instead of K more rounds.
                if (tid < K) run[cur ^ 1][tid] = kKeyEmpty;
                __syncthreads();
                for (int e = tid; e < 5 * K; e += kTopkThreads) {
                    const int l = e / K, j = e - l * K;
                    const key_t k = l < 4 ? wl[l][j] : run[cur][j];
                    if (k == kKeyEmpty) continue;
                    int rank = 0;
                    for (int i = 0; i < K; ++i)
                        rank += (wl[0][i] > k) + (wl[1][i] > k) + (wl[2][i] > k) + (wl[3][i] > k) + (run[cur][i] > k);
                    if (rank < K) run[cur ^ 1][rank] = k;
                }
            }
            cur ^= 1;
            __syncthreads();
        }
    } else {
        __shared__ key_t ls[kTopkMaxParts * kTopkMaxK];  // up to 63 lists of a pass
        const key_t* lists = static_cast<const key_t*>(src);
        for (long g0 = 0; g0 < N; g0 += kTopkMaxParts) {
            const int ng = (int)(N - g0 < kTopkMaxParts ? N - g0 : kTopkMaxParts);
            for (int e = tid; e < ng * K; e += kTopkThreads) {
                const int p = e / K;
                ls[e] = lists[((g0 + p) * B + b) * K + (e - p * K)];
            }
            __syncthreads();
            if (wave == 0) merge_heads(lane < ng ? ls + lane * K : lane == 63 ? run[cur] : nullptr, K, run[cur ^ 1]);
            cur ^= 1;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < K) dst[tid] = run[cur][tid];
}

// decode + gather for a list, one thread per (b, k): the list counterpart of select_rotation_kernel
__global__ __launch_bounds__(256) void select_topk_kernel(key_t* __restrict__ keys, int K, const float* __restrict__ R,
                                                          long r_batch_stride, long n_offset, long N, int B,
                                                          float* __restrict__ R_out, float* __restrict__ scores_out,
                                                          long* __restrict__ idx_out, bool reset)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * K) return;
    const int b = (int)(i / K);
    const key_t k = keys[i];
    if (reset) keys[i] = kKeyEmpty;
    const long gidx = (k == kKeyEmpty) ? -1l : key_index(k);
    if (scores_out) scores_out[i] = (k == kKeyEmpty) ? -INFINITY : key_score(k);
    if (idx_out) idx_out[i] = gidx;
    if (R_out) {
        const long loc = gidx - n_offset;
        const bool mine = (k != kKeyEmpty) && loc >= 0 && loc < N;  // sharded: the owner rank holds the row, the others zeros
        const float* r = R + (long)b * r_batch_stride + (mine ? loc : 0) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) R_out[i * 9 + e] = mine ? r[e] : 0.0f;
    }
}

// out[b][k * N2 + n] = R[idx_{b,k}] * D[n]: compose_rotations_kernel for K seeds (its expression, its in-bounds rule)
__global__ __launch_bounds__(256) void compose_rotations_topk_kernel(const key_t* __restrict__ keys, int K,
                                                                     const float* __restrict__ R, long r_batch_stride,
                                                                     long n_offset, long N, const float* __restrict__ D,
                                                                     long N2, int B, float* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * K * N2) return;
    const long bk = i / N2;  // b * K + k
    const long n = i - bk * N2;
    const int b = (int)(bk / K);
    const key_t key = keys[bk];
    long idx = key_index(key) - n_offset;
    idx = (key == kKeyEmpty || idx < 0 || idx >= N) ? 0 : idx;  // empty slot / foreign shard: stay in bounds
    const float* r = R + (long)b * r_batch_stride + idx * 9;
    const float* d = D + n * 9;
    float* o = out + i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = r[a * 3] * d[c] + r[a * 3 + 1] * d[3 + c] + r[a * 3 + 2] * d[6 + c];
}

// ---------------------------------------------------------------------------------
// Distinct pose modes (ahv_topk_modes_f32): greedy suppression by geodesic distance over the WHOLE scored set.  Entry j of
// the list is the largest key still alive; the winner then kills itself (by index, unconditionally) and every alive
// hypothesis i with t(i, w) = sum_ab R_i[a][b] R_w[a][b] >= tau (tau = 1 + 2 cos theta: for rotations "within theta of
// the winner").  A NaN t kills nothing.  K + 1 dependent launches: the list is filled EMPTY, round 0 packs the keys into the
// alive state, round j >= 1 applies winner j - 1 and reduces the largest survivor.  The KERNEL BOUNDARY is the hand-over of
// keys[j - 1]: no workgroup waits on another one.
// Alive state: the packed keys themselves, state[b][Ns] (Ns = N rounded up to 4) in the caller's workspace, kKeyEmpty =
// dead -- 8 bytes per hypothesis, read every round, written only where a hypothesis dies; the survivor's key needs no
// re-packing.  Grid rule of the top-K kernels: tiles of kTopkTile hypotheses, 256 threads, four consecutive hypotheses per
// lane; tile t starts at hypothesis t * kTopkTile.  A lane's four matrices are 144 contiguous bytes: nine 16-byte loads
// when THAT ADDRESS is 16-byte aligned (a per-sample R row with N % 4 != 0 starts mid-vector, so the tile index says
// nothing), element by element otherwise and at the ragged end.  A lane whose four hypotheses are all dead reads no
// matrix; a wave of such lanes issues no load.
// ---------------------------------------------------------------------------------
typedef long long i64x2 __attribute__((ext_vector_type(2)));

// the workgroup's largest key -> one atomicMax into *dst (skipped when nothing survives: *dst was filled kKeyEmpty)
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

// kFirst: round 0 -- state = pack_key(scores), keys[b][0] = the arg-max key.  !kFirst: round j.
template <bool kFirst>
__global__ __launch_bounds__(kTopkThreads) void topk_modes_kernel(const float* __restrict__ scores, const float* __restrict__ R,
                                                                  long r_batch_stride, long N, long Ns, long n_offset, int K,
                                                                  int j, float tau, key_t* __restrict__ state,
                                                                  key_t* __restrict__ keys)
{
    __shared__ key_t wl[kTopkThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    key_t* st = state + (long)b * Ns;
    key_t* list = keys + (long)b * K;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    key_t best = kKeyEmpty;
    if constexpr (kFirst) {
        const float* s = scores + (long)b * N;
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const long n0 = t * kTopkTile + (long)tid * 4;
            if (n0 >= N) continue;
            key_t c[4];
            if (n0 + 3 < N && (reinterpret_cast<unsigned long long>(s + n0) & 15ull) == 0) {
                const float4 q = *reinterpret_cast<const float4*>(s + n0);
                c[0] = pack_key(q.x, (unsigned)(n_offset + n0));
                c[1] = pack_key(q.y, (unsigned)(n_offset + n0 + 1));
                c[2] = pack_key(q.z, (unsigned)(n_offset + n0 + 2));
                c[3] = pack_key(q.w, (unsigned)(n_offset + n0 + 3));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) c[e] = n0 + e < N ? pack_key(s[n0 + e], (unsigned)(n_offset + n0 + e)) : kKeyEmpty;
            }
            // (the row is padded to Ns: all four slots exist; the padding is written dead)
            *reinterpret_cast<i64x2*>(st + n0) = i64x2{c[0], c[1]};
            *reinterpret_cast<i64x2*>(st + n0 + 2) = i64x2{c[2], c[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) best = c[e] > best ? c[e] : best;
        }
        modes_publish(best, wl, list);
    } else {
        const key_t prev = list[j - 1];
        if (prev == kKeyEmpty) return;  // the alive set ran out: keys[j..K) stay EMPTY (uniform over the grid)
        const long widx = key_index(prev) - n_offset;
        if (widx < 0 || widx >= N) return;  // (cannot happen for a list this call built: stay in bounds regardless)
        const float* Rb = R + (long)b * r_batch_stride;
        float w[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) w[i] = Rb[widx * 9 + i];
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const long n0 = t * kTopkTile + (long)tid * 4;
            if (n0 >= N) continue;
            const i64x2 c01 = *reinterpret_cast<const i64x2*>(st + n0), c23 = *reinterpret_cast<const i64x2*>(st + n0 + 2);
            key_t c[4] = {c01.x, c01.y, c23.x, c23.y};
            if (c[0] == kKeyEmpty && c[1] == kKeyEmpty && c[2] == kKeyEmpty && c[3] == kKeyEmpty) continue;
            const float* r = Rb + n0 * 9;
            float tr[4];
            if (n0 + 3 < N && (reinterpret_cast<unsigned long long>(r) & 15ull) == 0) {
                float4 q[9];
#pragma unroll
                for (int v = 0; v < 9; ++v) q[v] = reinterpret_cast<const float4*>(r)[v];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.0f;
#pragma unroll
                    for (int i = 0; i < 9; ++i) {
                        const int f = e * 9 + i;
                        const float4 v = q[f >> 2];
                        const float x = (f & 3) == 0 ? v.x : (f & 3) == 1 ? v.y : (f & 3) == 2 ? v.z : v.w;
                        acc = fmaf(x, w[i], acc);
                    }
                    tr[e] = acc;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float acc = 0.0f;
                    if (n0 + e < N && c[e] != kKeyEmpty) {
#pragma unroll
                        for (int i = 0; i < 9; ++i) acc = fmaf(r[e * 9 + i], w[i], acc);
                    }
                    tr[e] = acc;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c[e] == kKeyEmpty) continue;
                if (tr[e] >= tau || n0 + e == widx) {  // false for a NaN trace; the winner goes by its index
                    st[n0 + e] = kKeyEmpty;
                    continue;
                }
                best = c[e] > best ? c[e] : best;
            }
        }
        modes_publish(best, wl, list + j);
    }
}

// ---------------------------------------------------------------------------------
// Pose posterior (ahv_pose_posterior_f32 / _merge / _finish_f32): softmax statistics of the scored set at inverse temperature
// beta, split over K anchor buckets (hypothesis i belongs to the FIRST anchor k with t(i, k) >= tau, else to the rest).  What is
// kept per bucket and for the whole set is a RECORD of kPostRec doubles -- m (the largest score met, -inf when empty), and
// relative to it mass = sum w, S = sum w s, M = sum w R (9), w = exp((s - m) beta) -- so that two records merge by the
// online-softmax rule: m = max, each side rescaled by exp((m_side - m) beta).  A sample's STATE is a 16-byte header (int64
// n_excluded, int64 reserved) and K + 2 records: buckets 0 .. K-1, the rest bucket, the whole set.
//  - posterior_partial_kernel: ONE pass over scores and R on the grid rule of the top-K / modes kernels (tiles of kTopkTile,
//    four consecutive hypotheses per lane, 16-byte loads where THAT ADDRESS is aligned).  The anchors sit in LDS.  A lane keeps
//    online-softmax sums (fp32 weights, fp64 sums) for the whole set and the rest bucket; a mode bucket is hit rarely and is reduced wave-wide, only
//    when a ballot says some lane hit it, into the wave's LDS row in program order.  Wave sums are DPP row operations in fp64,
//    the four waves are combined in the order 0..3, one partial state per workgroup goes to the workspace.
//  - posterior_merge_kernel: states [P][B] -> state [B] in the order p = 0 .. P-1 (into the state, or from empty): the second
//    launch of a call and the merge after an all-gather.
//  - posterior_finish_kernel: a state -> the outputs; the rotation nearest to M is the top eigenvector of Horn's 4 x 4
//    quaternion matrix (the maximiser of sum R o M over SO(3) = U diag(1, 1, det(U V^T)) V^T), by cyclic Jacobi in fp64.
// No floating-point atomics: for a given (B, N, K) every sum is taken in one fixed order, so results are bitwise reproducible.
// ---------------------------------------------------------------------------------
constexpr int kPostMaxModes = 16;
constexpr int kPostRec = 12;      // doubles per record: m, mass, S, M[9]
constexpr int kPostHeader = 16;   // bytes: int64 n_excluded, int64 reserved (0)

__host__ __device__ constexpr size_t posterior_state_stride_dev(int K) { return (size_t)kPostHeader + (size_t)(K + 2) * kPostRec * sizeof(double); }
size_t posterior_state_stride(int K) { return posterior_state_stride_dev(K); }

int posterior_parts(int64_t N)
{
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    return (int)(tiles < kTopkMaxParts ? tiles : kTopkMaxParts);
}

struct PostAcc {  // one lane's online-softmax sums: the weights are fp32 (expf), the sums fp64 -- S / mass - m cancels, and an fp32
    float m;      // S would put its own rounding (times beta) into the entropy of a peaked distribution
    double mass, S, M[9];
};

__device__ __forceinline__ void post_clear(PostAcc& a)
{
    a.m = -INFINITY;
    a.mass = 0.0;
    a.S = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.M[i] = 0.0;
}

__device__ __forceinline__ void post_add(PostAcc& a, float s, const float* r, float beta)
{
    if (s > a.m) {  // a new maximum: rescale what is there (by 0 when nothing is: m = -inf)
        const double f = (double)expf((a.m - s) * beta);
        a.mass *= f;
        a.S *= f;
#pragma unroll
        for (int i = 0; i < 9; ++i) a.M[i] *= f;
        a.m = s;
    }
    const double w = (double)expf((s - a.m) * beta);
    a.mass += w;
    a.S = fma(w, (double)s, a.S);
#pragma unroll
    for (int i = 0; i < 9; ++i) a.M[i] = fma(w, (double)r[i], a.M[i]);
}

// dst <- dst merged with src (records of kPostRec doubles), dst's side first
__device__ __forceinline__ void post_merge(double* dst, const double* src, double beta)
{
    const double ma = dst[0], mb = src[0];
    const double m = mb > ma ? mb : ma;
    if (m == -INFINITY) return;  // both empty
    const double fa = ma == -INFINITY ? 0.0 : exp((ma - m) * beta), fb = mb == -INFINITY ? 0.0 : exp((mb - m) * beta);
    dst[0] = m;
#pragma unroll
    for (int i = 1; i < kPostRec; ++i) dst[i] = dst[i] * fa + src[i] * fb;
}

template <int kCtrl, int kRows, int kBanks>
__device__ __forceinline__ double sum_f64_dpp_step(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kCtrl, kRows, kBanks, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kCtrl, kRows, kBanks, true);
    return x + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// sum over the 64 lanes in the order of wave_sum_dpp, in fp64; valid in lane 63
__device__ __forceinline__ double wave_sum_dpp_f64(double x)
{
    x = sum_f64_dpp_step<0x111, 0xF, 0xF>(x);  // row_shr:1
    x = sum_f64_dpp_step<0x112, 0xF, 0xF>(x);  // row_shr:2
    x = sum_f64_dpp_step<0x114, 0xF, 0xE>(x);  // row_shr:4
    x = sum_f64_dpp_step<0x118, 0xF, 0xC>(x);  // row_shr:8
    x = sum_f64_dpp_step<0x142, 0xA, 0xF>(x);  // row_bcast:15
    x = sum_f64_dpp_step<0x143, 0xC, 0xF>(x);  // row_bcast:31
    return x;
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

// the 64 lanes' sums as one record, merged into row (LDS) by lane 63.  Called by whole waves only.
__device__ __forceinline__ void post_wave_into(const PostAcc& a, double beta, double* row)
{
    const float mw = wave_max_f32_dpp(a.m);
    const double f = a.m == -INFINITY ? 0.0 : exp(((double)a.m - (double)mw) * beta);
    double rec[kPostRec];
    rec[0] = (double)mw;
    rec[1] = wave_sum_dpp_f64(f * a.mass);
    rec[2] = wave_sum_dpp_f64(f * a.S);
#pragma unroll
    for (int i = 0; i < 9; ++i) rec[3 + i] = wave_sum_dpp_f64(f * a.M[i]);
    if ((threadIdx.x & 63) == 63) post_merge(row, rec, beta);
}

__global__ __launch_bounds__(kTopkThreads) void posterior_partial_kernel(const float* __restrict__ scores, const float* __restrict__ R,
                                                                         long r_batch_stride, int B, long N,
                                                                         const float* __restrict__ anchors, int K, float tau,
                                                                         float beta, char* __restrict__ partial)
{
    __shared__ double rows[kTopkThreads / 64][kPostMaxModes + 2][kPostRec];  // per wave: buckets, rest, whole
    __shared__ float anc[kPostMaxModes][9];
    __shared__ int used[kPostMaxModes];  // an all-zero anchor is an empty slot: skipped by this flag, not by its value
    __shared__ int n_excl;
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.y;
    const double beta_d = (double)beta;
    for (int e = tid; e < (kTopkThreads / 64) * (kPostMaxModes + 2) * kPostRec; e += kTopkThreads)
        (&rows[0][0][0])[e] = (e % kPostRec) == 0 ? (double)-INFINITY : 0.0;
    if (tid < K * 9) (&anc[0][0])[tid] = anchors[(long)b * K * 9 + tid];
    if (tid == 0) n_excl = 0;
    __syncthreads();
    if (tid < K) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) any = any || anc[tid][i] != 0.0f;  // true for a NaN entry: its t then matches nothing
        used[tid] = any ? 1 : 0;
    }
    __syncthreads();

    const float* s = scores + (long)b * N;
    const float* Rb = R + (long)b * r_batch_stride;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    PostAcc whole, rest;
    post_clear(whole);
    post_clear(rest);
    int excluded = 0;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform over the workgroup: every lane takes every trip)
        const long n0 = t * kTopkTile + (long)tid * 4;
        float sc[4], r[4][9];
        int bk[4];  // K: rest, k < K: bucket k, -1: no such hypothesis / not in the scored set
        const bool full = n0 + 3 < N;
        if (full && (reinterpret_cast<unsigned long long>(s + n0) & 15ull) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(s + n0);
            sc[0] = q.x; sc[1] = q.y; sc[2] = q.z; sc[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) sc[e] = n0 + e < N ? s[n0 + e] : 0.0f;
        }
        const float* rp = Rb + n0 * 9;
        if (full && (reinterpret_cast<unsigned long long>(rp) & 15ull) == 0) {
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
                for (int i = 0; i < 9; ++i) r[e][i] = n0 + e < N ? rp[e * 9 + i] : 0.0f;
        }
        bool hit = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool exists = n0 + e < N;
            const bool scored = exists && fabsf(sc[e]) < __builtin_inff();  // false for NaN and +-inf
            excluded += (exists && !scored) ? 1 : 0;
            bk[e] = scored ? K : -1;
        }
        for (int k = K - 1; k >= 0; --k) {  // descending: the FIRST matching anchor is the one left standing
            if (!used[k]) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 9; ++i) acc = fmaf(r[e][i], anc[k][i], acc);
                bk[e] = (bk[e] >= 0 && acc >= tau) ? k : bk[e];  // false for a NaN t
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (bk[e] < 0) continue;
            post_add(whole, sc[e], r[e], beta);
            if (bk[e] == K) post_add(rest, sc[e], r[e], beta);
            else hit = true;
        }
        if (__ballot(hit)) {  // rare (a 15-degree cap holds 0.1 % of SO(3)); wave-uniform from here on
            for (int k = 0; k < K; ++k) {
                const bool mine = bk[0] == k || bk[1] == k || bk[2] == k || bk[3] == k;
                if (!__ballot(mine)) continue;
                PostAcc a;
                post_clear(a);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (bk[e] == k) post_add(a, sc[e], r[e], beta);
                post_wave_into(a, beta_d, rows[wave][k]);
            }
        }
    }
    post_wave_into(rest, beta_d, rows[wave][K]);
    post_wave_into(whole, beta_d, rows[wave][K + 1]);
    if (excluded) atomicAdd(&n_excl, excluded);  // an integer count: order does not matter
    __syncthreads();
    char* st = partial + ((size_t)blockIdx.x * B + b) * posterior_state_stride_dev(K);
    if (tid < K + 2) {  // the four waves in the order 0..3
        double rec[kPostRec];
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) rec[i] = rows[0][tid][i];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) post_merge(rec, rows[w][tid], beta_d);
        double* dst = reinterpret_cast<double*>(st + kPostHeader) + tid * kPostRec;
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) dst[i] = rec[i];
    }
    if (tid == 63) {
        reinterpret_cast<long long*>(st)[0] = n_excl;
        reinterpret_cast<long long*>(st)[1] = 0;
    }
}

// states [P][B] -> state [B], in the order p = 0 .. P-1; carry: state's own content comes first
__global__ __launch_bounds__(64) void posterior_merge_kernel(const char* __restrict__ states, int P, int B, int K, float beta,
                                                             char* __restrict__ state, bool carry)
{
    const int b = blockIdx.x, j = threadIdx.x;
    const size_t stride = posterior_state_stride_dev(K);
    char* dst = state + (size_t)b * stride;
    if (j < K + 2) {
        double* d = reinterpret_cast<double*>(dst + kPostHeader) + j * kPostRec;
        double rec[kPostRec];
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) rec[i] = carry ? d[i] : (i == 0 ? (double)-INFINITY : 0.0);
        for (int p = 0; p < P; ++p) {
            const double* src = reinterpret_cast<const double*>(states + ((size_t)p * B + b) * stride + kPostHeader) + j * kPostRec;
            double in[kPostRec];
#pragma unroll
            for (int i = 0; i < kPostRec; ++i) in[i] = src[i];
            post_merge(rec, in, (double)beta);
        }
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) d[i] = rec[i];
    }
    if (j == 63) {
        long long n = carry ? reinterpret_cast<const long long*>(dst)[0] : 0;
        for (int p = 0; p < P; ++p) n += reinterpret_cast<const long long*>(states + ((size_t)p * B + b) * stride)[0];
        reinterpret_cast<long long*>(dst)[0] = n;
        reinterpret_cast<long long*>(dst)[1] = 0;
    }
}

// one Jacobi rotation of the symmetric A (4 x 4) in the (P, Q) plane, accumulated into V
template <int P, int Q>
__device__ __forceinline__ void jacobi4_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// Rm = the rotation nearest to M (Frobenius), spread = the angle whose cosine is (sum Rm o M - 1) / 2, in degrees.
// M is a weighted mean of the matrices (already divided by the mass).
__device__ __forceinline__ void post_project(const double* M, float* Rm, float* spread)
{
    double A[4][4] = {{M[0] + M[4] + M[8], M[7] - M[5], M[2] - M[6], M[3] - M[1]},
                      {M[7] - M[5], M[0] - M[4] - M[8], M[1] + M[3], M[2] + M[6]},
                      {M[2] - M[6], M[1] + M[3], -M[0] + M[4] - M[8], M[5] + M[7]},
                      {M[3] - M[1], M[2] + M[6], M[5] + M[7], -M[0] - M[4] + M[8]}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {  // cyclic Jacobi converges quadratically: 12 sweeps are far past fp64 for a 4 x 4
        jacobi4_rotate<0, 1>(A, V);
        jacobi4_rotate<0, 2>(A, V);
        jacobi4_rotate<0, 3>(A, V);
        jacobi4_rotate<1, 2>(A, V);
        jacobi4_rotate<1, 3>(A, V);
        jacobi4_rotate<2, 3>(A, V);
    }
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool take = A[c][c] > best;
        best = take ? A[c][c] : best;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = take ? V[k][c] : q[k];
    }
    const double nn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * nn, x = q[1] * nn, y = q[2] * nn, z = q[3] * nn;
    const double Rd[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                          2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                          2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) dot += Rd[i] * M[i];
    double cs = (dot - 1.0) * 0.5;
    cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;  // (a NaN stays a NaN)
    if (Rm) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Rm[i] = (float)Rd[i];
    }
    if (spread) *spread = (float)(acos(cs) * 57.295779513082320877);
}

// thread j of block b: bucket j < K, the rest bucket (j = K) or the whole set (j = K + 1)
__global__ __launch_bounds__(64) void posterior_finish_kernel(const char* __restrict__ state, int B, int K, float beta,
                                                              float* __restrict__ log_z, float* __restrict__ entropy,
                                                              float* __restrict__ mean_score, long long* __restrict__ n_excluded,
                                                              float* __restrict__ mode_prob, float* __restrict__ rest_prob,
                                                              float* __restrict__ mode_R_mean, float* __restrict__ R_mean,
                                                              float* __restrict__ mode_spread, float* __restrict__ spread)
{
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= K + 2) return;
    const char* st = state + (size_t)b * posterior_state_stride_dev(K);
    const double* recs = reinterpret_cast<const double*>(st + kPostHeader);
    const double* all = recs + (K + 1) * kPostRec;
    const double* me = recs + j * kPostRec;
    const double bd = (double)beta, m_all = all[0], Z = all[1];
    const bool empty = !(me[1] > 0.0);  // an empty slot, a bucket without a member, an empty scored set
    if (j == K + 1) {
        if (n_excluded) n_excluded[b] = reinterpret_cast<const long long*>(st)[0];
        if (log_z) log_z[b] = empty ? -INFINITY : (float)(m_all * bd + log(Z));
        if (entropy) entropy[b] = empty ? __builtin_nanf("") : (float)(log(Z) - bd * (all[2] / Z - m_all));
        if (mean_score) mean_score[b] = empty ? __builtin_nanf("") : (float)(all[2] / Z);
    } else {
        const float p = empty ? 0.0f : (float)(me[1] * exp((me[0] - m_all) * bd) / Z);
        if (j == K) {
            if (rest_prob) rest_prob[b] = p;
            return;
        }
        if (mode_prob) mode_prob[(long)b * K + j] = p;
    }
    float* Rm = j <= K ? (mode_R_mean ? mode_R_mean + ((long)b * K + j) * 9 : nullptr) : (R_mean ? R_mean + (long)b * 9 : nullptr);
    float* sp = j <= K ? (mode_spread ? mode_spread + (long)b * K + j : nullptr) : (spread ? spread + b : nullptr);
    if (!Rm && !sp) return;
    if (empty) {
        if (Rm) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Rm[i] = 0.0f;
        }
        if (sp) *sp = __builtin_nanf("");
        return;
    }
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = me[3 + i] / me[1];
    post_project(M, Rm, sp);
}

// ---------------------------------------------------------------------------------
// Haar-uniform rotation hypotheses generated on the device (replaces the host call
// pytorch3d.transforms.random_rotations(N), test_co3d.py:106 / modules/model.py:184; only the
// distribution matters -- hypotheses are inputs of the hot path).  Counter-based: rotation n
// depends on (seed, offset + n) alone, so any shard of the set can be generated anywhere,
// reproducibly, and the call is graph-capturable.  Philox-4x32-10 -> 4 uniforms -> Box-Muller
// -> normalised Gaussian quaternion -> matrix.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(256) void random_rotations_kernel(unsigned long long seed, unsigned long long offset, long N,
                                                               float* __restrict__ out)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const unsigned long long ctr = offset + (unsigned long long)n;
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0x3D4148u, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    // uniforms in (0,1]: never log(0)
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u1, &s0, &c0);
    sincosf(6.28318530717958647692f * u3, &s1, &c1);
    const float qr = r0 * c0, qi = r0 * s0, qj = r1 * c1, qk = r1 * s1;
    const float t = 2.0f / fmaxf(qr * qr + qi * qi + qj * qj + qk * qk, 1e-30f);
    float* o = out + n * 9;
    o[0] = 1.0f - t * (qj * qj + qk * qk); o[1] = t * (qi * qj - qk * qr);        o[2] = t * (qi * qk + qj * qr);
    o[3] = t * (qi * qj + qk * qr);        o[4] = 1.0f - t * (qi * qi + qk * qk); o[5] = t * (qj * qk - qi * qr);
    o[6] = t * (qi * qk - qj * qr);        o[7] = t * (qj * qk + qi * qr);        o[8] = 1.0f - t * (qi * qi + qj * qj);
}

// Super-Fibonacci SO(3) grid (Alexa, CVPR 2022): point i of n is the quaternion
// (sqrt(t) sin a, sqrt(t) cos a, sqrt(1-t) sin b, sqrt(1-t) cos b), t = (i + 1/2)/n, a = 2 pi (i + 1/2)/sqrt(2),
// b = 2 pi (i + 1/2)/psi.  The angles reach 10^6 rad, so their turn fraction is taken in fp64 before sin/cos.
__global__ __launch_bounds__(256) void so3_grid_kernel(long n_total, long offset, long N, float* __restrict__ out)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const double s = (double)(offset + n) + 0.5;
    const double t = s / (double)n_total;
    double fa = s * 0.70710678118654752440, fb = s * (1.0 / 1.533751168755204288118041);
    fa -= floor(fa);
    fb -= floor(fb);
    float sa, ca, sb, cb;
    sincosf(6.28318530717958647692f * (float)fa, &sa, &ca);
    sincosf(6.28318530717958647692f * (float)fb, &sb, &cb);
    const float r = sqrtf((float)t), Rr = sqrtf((float)(1.0 - t));
    const float qr = r * sa, qi = r * ca, qj = Rr * sb, qk = Rr * cb;  // unit norm by construction
    float* o = out + n * 9;
    o[0] = 1.0f - 2.0f * (qj * qj + qk * qk); o[1] = 2.0f * (qi * qj - qk * qr);        o[2] = 2.0f * (qi * qk + qj * qr);
    o[3] = 2.0f * (qi * qj + qk * qr);        o[4] = 1.0f - 2.0f * (qi * qi + qk * qk); o[5] = 2.0f * (qj * qk - qi * qr);
    o[6] = 2.0f * (qi * qk - qj * qr);        o[7] = 2.0f * (qj * qk + qi * qr);        o[8] = 1.0f - 2.0f * (qi * qi + qj * qj);
}

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_rotate_volume(const float* vol, int64_t vol_batch_stride, const float* R, int64_t N, int C,
                                int D, int H, int W, float* out, int num_cu, hipStream_t stream)
{
    if (C == 16 && D == 8 && H == 8 && W == 8 && vol_batch_stride == 0) {
        long blocks = (N + 3) / 4;
        const long cap = (long)num_cu * 3;  // 47.5 KiB of LDS per workgroup: three per CU are resident
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(rotate_volume_16x8_kernel, dim3((unsigned)blocks), dim3(kRotThreads), 0, stream, vol,
                           R, (long)N, out);
    } else {
        const long total = (long)N * D * H * W;
        long blocks = (total + 255) / 256;
        const long cap = (long)num_cu * 16;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(rotate_volume_generic_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, vol,
                           (long)vol_batch_stride, R, (long)N, C, D, H, W, out);
    }
    return hipGetLastError();
}

hipError_t launch_rotate_volume_backward(const float* grad_out, int64_t vol_batch_stride, const float* R, int64_t N,
                                         int C, int D, int H, int W, float* grad_vol, int num_cu, hipStream_t stream)
{
    const long total = (long)N * D * H * W;
    long blocks = (total + 255) / 256;
    const long cap = (long)num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rotate_volume_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, grad_out,
                       (long)vol_batch_stride, R, (long)N, C, D, H, W, grad_vol);
    return hipGetLastError();
}

hipError_t launch_forward_3d2d(const float* vol, const float* W1, const float* W2, const float* b2, int64_t M,
                               float* out, int num_cu, hipStream_t stream)
{
    const size_t lds = sizeof(float) * kF32LdsFloats;
    static thread_local int attr_dev = -1;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (attr_dev != dev) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(forward_3d2d_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_dev = dev;
    }
    if (M <= 64) {  // latency path: one workgroup per item, quarters and slabs split over its 8 waves
        hipLaunchKernelGGL(forward_3d2d_small_kernel, dim3((unsigned)M), dim3(512), 0, stream, vol, W1, W2, b2, out);
        return hipGetLastError();
    }
    if (M >= 4096) {  // throughput path
        long blocks = (M + 7) / 8;
        if (blocks > num_cu) blocks = num_cu;
        hipLaunchKernelGGL(forward_3d2d_dual_kernel, dim3((unsigned)blocks), dim3(512), 0, stream, vol, W1, W2, b2,
                           (long)M, out);
        return hipGetLastError();
    }
    long blocks = (M + 3) / 4;
    if (blocks > num_cu) blocks = num_cu;
    hipLaunchKernelGGL(forward_3d2d_kernel, dim3((unsigned)blocks), dim3(kF32Threads), lds, stream, vol, W1, W2,
                       b2, (long)M, out);
    return hipGetLastError();
}

hipError_t launch_score_features(const float* f_src, const float* f_tgt, int B, int64_t N, float* scores,
                                 int num_cu, hipStream_t stream)
{
    long blocks = ((long)B * N + 3) / 4;
    const long cap = (long)num_cu * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(score_features_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, f_src, f_tgt, B,
                       (long)N, scores);
    return hipGetLastError();
}

hipError_t launch_compose_rotations(const int64_t* best_key, const float* R, int64_t r_batch_stride,
                                    int64_t n_offset, int64_t N, const float* D, int64_t N2, int B, float* out,
                                    hipStream_t stream)
{
    const long total = (long)B * N2;
    hipLaunchKernelGGL(compose_rotations_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const key_t*>(best_key), R, (long)r_batch_stride, (long)n_offset, (long)N, D,
                       (long)N2, B, out);
    return hipGetLastError();
}

hipError_t launch_select_rotation(int64_t* best_key, const float* R, int64_t r_batch_stride, int64_t n_offset,
                                  int64_t N, int B, float* R_out, float* best_score, int64_t* best_idx, bool reset,
                                  hipStream_t stream)
{
    hipLaunchKernelGGL(select_rotation_kernel, dim3((B + 63) / 64), dim3(64), 0, stream,
                       reinterpret_cast<key_t*>(best_key), R, (long)r_batch_stride, (long)n_offset, (long)N, B, R_out,
                       best_score, reinterpret_cast<long*>(best_idx), reset);
    return hipGetLastError();
}

hipError_t launch_random_rotations(uint64_t seed, uint64_t offset, int64_t N, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(random_rotations_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream,
                       (unsigned long long)seed, (unsigned long long)offset, (long)N, out);
    return hipGetLastError();
}

hipError_t launch_so3_grid(int64_t n_total, int64_t offset, int64_t N, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(so3_grid_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (long)n_total,
                       (long)offset, (long)N, out);
    return hipGetLastError();
}

hipError_t launch_argmax(const float* scores, int B, int64_t N, int64_t n_offset, int64_t* best_key,
                         int num_cu, hipStream_t stream)
{
    long bx = (N + 255) / 256;
    const long cap = num_cu * 4 / (B < num_cu ? B : num_cu) + 1;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, scores, B, (long)N,
                       (long)n_offset, reinterpret_cast<key_t*>(best_key));
    return hipGetLastError();
}

// partial lists per sample of a top-K launch over N scores: a pure function of N (the workspace is sized by it)
int topk_parts(int64_t N)
{
    const int64_t tiles = (N + 3 + kTopkTile - 1) / kTopkTile;  // + 3: the row may start up to three floats past a 16-byte line
    return (int)(tiles < kTopkMaxParts ? tiles : kTopkMaxParts);
}

hipError_t launch_topk_merge(const int64_t* lists, int P, int B, int K, int64_t* keys, bool carry, hipStream_t stream)
{
    hipLaunchKernelGGL(topk_kernel<false>, dim3(1, (unsigned)B), dim3(kTopkThreads), 0, stream,
                       static_cast<const void*>(lists), B, (long)P, 0l, K, reinterpret_cast<key_t*>(keys), carry);
    return hipGetLastError();
}

hipError_t launch_topk(const float* scores, int B, int64_t N, int64_t n_offset, int K, int64_t* keys, int64_t* workspace,
                       bool carry, hipStream_t stream)
{
    const int parts = topk_parts(N);
    if (parts <= 1) {  // one tile: straight into the caller's list
        hipLaunchKernelGGL(topk_kernel<true>, dim3(1, (unsigned)B), dim3(kTopkThreads), 0, stream,
                           static_cast<const void*>(scores), B, (long)N, (long)n_offset, K, reinterpret_cast<key_t*>(keys),
                           carry);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(topk_kernel<true>, dim3((unsigned)parts, (unsigned)B), dim3(kTopkThreads), 0, stream,
                       static_cast<const void*>(scores), B, (long)N, (long)n_offset, K,
                       reinterpret_cast<key_t*>(workspace), false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_topk_merge(workspace, parts, B, K, keys, carry, stream);
}

hipError_t launch_select_topk(int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset, int64_t N,
                              int B, float* R_out, float* scores_out, int64_t* idx_out, bool reset, hipStream_t stream)
{
    const long total = (long)B * K;
    hipLaunchKernelGGL(select_topk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<key_t*>(keys), K, R, (long)r_batch_stride, (long)n_offset, (long)N, B, R_out,
                       scores_out, reinterpret_cast<long*>(idx_out), reset);
    return hipGetLastError();
}

hipError_t launch_compose_rotations_topk(const int64_t* keys, int K, const float* R, int64_t r_batch_stride,
                                         int64_t n_offset, int64_t N, const float* D, int64_t N2, int B, float* out,
                                         hipStream_t stream)
{
    const long total = (long)B * K * N2;
    hipLaunchKernelGGL(compose_rotations_topk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const key_t*>(keys), K, R, (long)r_batch_stride, (long)n_offset, (long)N, D,
                       (long)N2, B, out);
    return hipGetLastError();
}

// best_key[0..B) = EMPTY (below every real key): one tiny launch, graph-capturable
__global__ void fill_keys_kernel(key_t* __restrict__ k, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) k[b] = kKeyEmpty;
}

hipError_t launch_fill_keys(int64_t* best_key, int B, hipStream_t stream)
{
    hipLaunchKernelGGL(fill_keys_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, reinterpret_cast<key_t*>(best_key), B);
    return hipGetLastError();
}

// hypotheses per sample of the alive state of ahv_topk_modes_f32: N rounded up to a lane's four
int64_t topk_modes_state_stride(int64_t N) { return (N + 3) & ~(int64_t)3; }

// K + 1 launches: the list filled EMPTY, round 0, rounds 1 .. K - 1 (each reads the entry the one before reduced)
hipError_t launch_topk_modes(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                             int K, float tau, int64_t* keys, int64_t* state, hipStream_t stream)
{
    hipError_t e = launch_fill_keys(keys, B * K, stream);
    if (e != hipSuccess) return e;
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    const long Ns = (long)topk_modes_state_stride(N);
    hipLaunchKernelGGL(topk_modes_kernel<true>, grid, dim3(kTopkThreads), 0, stream, scores, R, (long)r_batch_stride, (long)N,
                       Ns, (long)n_offset, K, 0, tau, reinterpret_cast<key_t*>(state), reinterpret_cast<key_t*>(keys));
    for (int j = 1; j < K; ++j)
        hipLaunchKernelGGL(topk_modes_kernel<false>, grid, dim3(kTopkThreads), 0, stream, scores, R, (long)r_batch_stride,
                           (long)N, Ns, (long)n_offset, K, j, tau, reinterpret_cast<key_t*>(state),
                           reinterpret_cast<key_t*>(keys));
    return hipGetLastError();
}

// ---- pose posterior ---------------------------------------------------------------------------------------
hipError_t launch_posterior_merge(const void* states, int P, int B, int K, float beta, void* state, bool carry, hipStream_t stream)
{
    hipLaunchKernelGGL(posterior_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, static_cast<const char*>(states), P, B, K,
                       beta, static_cast<char*>(state), carry);
    return hipGetLastError();
}

// two launches: one partial state per workgroup into the workspace, then their merge into (or over) the caller's state
hipError_t launch_posterior(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, const float* anchors,
                            int K, float tau, float beta, void* state, void* workspace, bool carry, hipStream_t stream)
{
    const int parts = posterior_parts(N);
    hipLaunchKernelGGL(posterior_partial_kernel, dim3((unsigned)parts, (unsigned)B), dim3(kTopkThreads), 0, stream, scores, R,
                       (long)r_batch_stride, B, (long)N, anchors, K, tau, beta, static_cast<char*>(workspace));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_posterior_merge(workspace, parts, B, K, beta, state, carry, stream);
}

hipError_t launch_posterior_finish(const void* state, int B, int K, float beta, float* log_z, float* entropy, float* mean_score,
                                   int64_t* n_excluded, float* mode_prob, float* rest_prob, float* mode_R_mean, float* R_mean,
                                   float* mode_spread_deg, float* spread_deg, hipStream_t stream)
{
    hipLaunchKernelGGL(posterior_finish_kernel, dim3((unsigned)B), dim3(64), 0, stream, static_cast<const char*>(state), B, K, beta,
                       log_z, entropy, mean_score, reinterpret_cast<long long*>(n_excluded), mode_prob, rest_prob, mode_R_mean,
                       R_mean, mode_spread_deg, spread_deg);
    return hipGetLastError();
}

// ---- zero fill ------------------------------------------------------------------------------------------
// The library's accumulation targets (gradients, best keys) are zeroed by THIS kernel, not by hipMemsetAsync: a run
// of memset nodes captured into a hipGraph (six in front of the scorer backward) did not reliably take effect on
// replay on ROCm 7.2 -- replay 0 was right because fresh pool memory is zero, every later replay accumulated onto
// whatever the pool block held (tests/test_gpu_graph_replay.py).  One launch for up to six spans.
struct ZeroSpans {
    void* p[6];
    unsigned long long bytes[6];  // multiples of 4
};

__global__ __launch_bounds__(256) void zero_fill_kernel(const ZeroSpans a)
{
    const unsigned long long i0 = (unsigned long long)blockIdx.x * 256 + threadIdx.x, step = (unsigned long long)gridDim.x * 256;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long nb = a.bytes[k];
        if (nb == 0) continue;
        unsigned long long n16 = (reinterpret_cast<unsigned long long>(a.p[k]) & 15) ? 0 : nb >> 4;
        uint4* q = static_cast<uint4*>(a.p[k]);
        for (unsigned long long i = i0; i < n16; i += step) q[i] = uint4{0u, 0u, 0u, 0u};
        unsigned* d = static_cast<unsigned*>(a.p[k]) + 4 * n16;
        const unsigned long long nd = (nb >> 2) - 4 * n16;
        for (unsigned long long i = i0; i < nd; i += step) d[i] = 0u;
    }
}

hipError_t launch_zero_fill(void* const* ptrs, const size_t* bytes, int count, hipStream_t stream)
{
    if (count < 0 || count > 6) return hipErrorInvalidValue;
    ZeroSpans a;
    unsigned long long most = 0;
    for (int k = 0; k < 6; ++k) {
        a.p[k] = k < count ? ptrs[k] : nullptr;
        a.bytes[k] = (k < count && ptrs[k]) ? bytes[k] : 0;
        if (a.bytes[k] & 3) return hipErrorInvalidValue;
        if (a.bytes[k] > most) most = a.bytes[k];
    }
    if (most == 0) return hipSuccess;
    unsigned long long blocks = (most / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- SO(3) ascent step (ahv_so3_ascent_candidates_f32 / ahv_so3_ascent_select_f32) ----------------------
// One thread per seed (b, k); rotations.so3_ascent_candidates / so3_ascent_select state the same rules in torch.
// Direction: the Riemannian gradient in the body frame, w = vee(1/2 (R^T G - G^T R)); candidate slot 0 is R_cur bit for bit,
// slot l >= 1 is R_cur exp(ladder[l-1] theta [w / |w|]x) (Rodrigues, 1 - cos a as 2 sin^2(a / 2)); |w| = 0 or a non-finite w:
// every slot is R_cur.
__global__ __launch_bounds__(256) void so3_ascent_candidates_kernel(const float* __restrict__ R_cur, const float* __restrict__ grad_R,
                                                                    const float* __restrict__ theta, const float* __restrict__ ladder,
                                                                    int L, int seeds, float* __restrict__ R_cand)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= seeds) return;
    float R[9], G[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        R[j] = R_cur[(long)i * 9 + j];
        G[j] = grad_R[(long)i * 9 + j];
    }
    float A[9];   // R^T G
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = R[r] * G[c] + R[3 + r] * G[3 + c] + R[6 + r] * G[6 + c];
    const float wx = 0.5f * (A[7] - A[5]), wy = 0.5f * (A[2] - A[6]), wz = 0.5f * (A[3] - A[1]);
    const float nrm = sqrtf(wx * wx + wy * wy + wz * wz);
    const bool move = nrm > 0.0f && nrm < __builtin_inff();   // false for NaN
    const float inv = move ? 1.0f / nrm : 0.0f;
    const float nx = wx * inv, ny = wy * inv, nz = wz * inv;
    const float th = theta[i];
    float* out = R_cand + (long)i * (L + 1) * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) out[j] = R[j];
    for (int l = 1; l <= L; ++l) {
        float* o = out + l * 9;
        if (!move) {
#pragma unroll
            for (int j = 0; j < 9; ++j) o[j] = R[j];
            continue;
        }
        const float a = ladder[l - 1] * th;
        const float sn = sinf(a), sh = sinf(0.5f * a), c1 = 2.0f * sh * sh;
        // E = I + sin a K + (1 - cos a) (n n^T - I), K = [n]x
        const float E[9] = {1.0f + c1 * (nx * nx - 1.0f), c1 * nx * ny - sn * nz, c1 * nx * nz + sn * ny,
                            c1 * nx * ny + sn * nz, 1.0f + c1 * (ny * ny - 1.0f), c1 * ny * nz - sn * nx,
                            c1 * nx * nz - sn * ny, c1 * ny * nz + sn * nx, 1.0f + c1 * (nz * nz - 1.0f)};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * r + c] = R[3 * r] * E[c] + R[3 * r + 1] * E[3 + c] + R[3 * r + 2] * E[6 + c];
    }
}

// A candidate replaces the incumbent only if its score is strictly greater (false for NaN), slots scanned in order: a seed's
// score never decreases, slot 0 (R_cur itself) wins a tie.  theta <- ladder[l-1] theta for the accepted slot, theta min(ladder)
// when slot 0 stayed.
__global__ __launch_bounds__(256) void so3_ascent_select_kernel(const float* __restrict__ R_cand, const float* __restrict__ cand_scores,
                                                                const float* __restrict__ ladder, int L, int seeds,
                                                                float* __restrict__ R_cur, float* __restrict__ score_cur,
                                                                float* __restrict__ theta)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= seeds) return;
    const float* sc = cand_scores + (long)i * (L + 1);
    float best = sc[0], lmin = ladder[0];
    int slot = 0;
    for (int l = 1; l <= L; ++l) {
        const float s = sc[l];
        if (s > best) {
            best = s;
            slot = l;
        }
        lmin = fminf(lmin, ladder[l - 1]);
    }
    const float* src = R_cand + ((long)i * (L + 1) + slot) * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) R_cur[(long)i * 9 + j] = src[j];
    score_cur[i] = best;
    theta[i] = theta[i] * (slot ? ladder[slot - 1] : lmin);
}

hipError_t launch_so3_ascent_candidates(const float* R_cur, const float* grad_R, const float* theta, const float* ladder, int L,
                                        int B, int K, float* R_cand, hipStream_t stream)
{
    const int seeds = B * K;
    if (seeds == 0) return hipSuccess;
    hipLaunchKernelGGL(so3_ascent_candidates_kernel, dim3((seeds + 255) / 256), dim3(256), 0, stream, R_cur, grad_R, theta,
                       ladder, L, seeds, R_cand);
    return hipGetLastError();
}

hipError_t launch_so3_ascent_select(const float* R_cand, const float* cand_scores, const float* ladder, int L, int B, int K,
                                    float* R_cur, float* score_cur, float* theta, hipStream_t stream)
{
    const int seeds = B * K;
    if (seeds == 0) return hipSuccess;
    hipLaunchKernelGGL(so3_ascent_select_kernel, dim3((seeds + 255) / 256), dim3(256), 0, stream, R_cand, cand_scores, ladder,
                       L, seeds, R_cur, score_cur, theta);
    return hipGetLastError();
}

}  // namespace ahv
