// ahv_ops.hip -- op-level drop-in kernels: each materialises the tensor the
// reference's corresponding call returns, so the reference's own call sequence
// (rotate_volume -> forward_3d2d -> mul/sum/mean -> max) runs unchanged on HIP.
// These are the HBM-bound siblings of the fused scorer (ahv_score.hip).  Also here: the hypothesis generators
// (random_rotations, so3_grid) and the library's zero fill.  What happens once the scores exist -- the arg-max of that
// sequence, lists, modes, posterior, ascent -- is ahv_select.hip.
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

// (qr, qi, qj, qk) of any norm > 0 -> the nine matrix entries at o
__device__ __forceinline__ void quaternion_matrix(float qr, float qi, float qj, float qk, float* __restrict__ o)
{
    const float t = 2.0f / fmaxf(qr * qr + qi * qi + qj * qj + qk * qk, 1e-30f);
    o[0] = 1.0f - t * (qj * qj + qk * qk); o[1] = t * (qi * qj - qk * qr);        o[2] = t * (qi * qk + qj * qr);
    o[3] = t * (qi * qj + qk * qr);        o[4] = 1.0f - t * (qi * qi + qk * qk); o[5] = t * (qj * qk - qi * qr);
    o[6] = t * (qi * qk - qj * qr);        o[7] = t * (qj * qk + qi * qr);        o[8] = 1.0f - t * (qi * qi + qj * qj);
}

// Four uniforms of one Philox block -> two Box-Muller pairs (g0, g1), (g2, g3): standard normal, independent.
__device__ __forceinline__ void box_muller4(const unsigned (&c)[4], float& g0, float& g1, float& g2, float& g3)
{
    // uniforms in (0,1]: never log(0)
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u1, &s0, &c0);
    sincosf(6.28318530717958647692f * u3, &s1, &c1);
    g0 = r0 * c0; g1 = r0 * s0; g2 = r1 * c1; g3 = r1 * s1;
}

// Rotation `ctr` of the Haar stream of `seed`: what ahv_random_rotations_f32 writes for offset + n = ctr, bit for bit
// (random_rotations_kernel and the fresh slots of diffuse_rotations_kernel both call it).
__device__ __noinline__ void haar_rotation(unsigned long long seed, unsigned long long ctr, float* __restrict__ o)
{
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0x3D4148u, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    float qr, qi, qj, qk;
    box_muller4(c, qr, qi, qj, qk);
    quaternion_matrix(qr, qi, qj, qk, o);
}

__global__ __launch_bounds__(256) void random_rotations_kernel(unsigned long long seed, unsigned long long offset, long N,
                                                               float* __restrict__ out)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    haar_rotation(seed, offset + (unsigned long long)n, out + n * 9);
}

// ---------------------------------------------------------------------------------
// Particle-filter predict step (ahv_diffuse_rotations_f32, include/ahv.h): one thread per slot (b, j) of the new set.
//   elite  j == 0 with a key: R[b][decode(key_b)] copied bit for bit
//   fresh  j >= M - n_fresh: rotation (step B + b) M + j of the Haar stream of seed ^ kFreshSeed
//   else   R[b][idx[b][j]] exp([w]x), w = sigma z clipped to max_angle, composed as unit quaternions and normalised, so that
//          a set fed back for thousands of steps stays on SO(3)
// The noise block of a slot is Philox(key = seed, counter = (j, b | step[47:32] << 16, kDiffuseTag, step[31:0])): a function of
// (seed, step mod 2^48, b, j) alone, and never a block of the Haar stream (word 2 differs).  `step` is read on the device.
// ---------------------------------------------------------------------------------
constexpr unsigned long long kFreshSeed = 0x9E3779B97F4A7C15ull;
constexpr unsigned kDiffuseTag = 0x444946u, kAdvanceTag = 0x414456u;

__global__ __launch_bounds__(256) void diffuse_rotations_kernel(const long long* __restrict__ idx, const float* __restrict__ R,
                                                                long r_batch_stride, long N, const key_t* __restrict__ best_key,
                                                                long M, long n_fresh, unsigned long long seed,
                                                                const long long* __restrict__ step, float sigma, float max_angle,
                                                                float* __restrict__ out, float* __restrict__ omega)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const long b = blockIdx.y;
    const unsigned long long t = (unsigned long long)*step;
    const long i = b * M + j;
    float* o = out + i * 9;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
    if (j == 0 && best_key) {
        const key_t key = best_key[b];
        long n = key_index(key);
        n = (key == kKeyEmpty || n < 0 || n >= N) ? 0 : n;  // as compose_rotations_topk_kernel: stay in bounds
        const float* r = R + b * r_batch_stride + n * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = r[k];
    } else if (j >= M - n_fresh) {
        haar_rotation(seed ^ kFreshSeed, (t * (unsigned long long)gridDim.y + (unsigned long long)b) * (unsigned long long)M + (unsigned long long)j, o);
    } else {
        long n = idx ? (long)idx[i] : j % N;
        n = (n < 0 || n >= N) ? 0 : n;  // -1 (a sample without a finite score) or a foreign list: stay in bounds
        const float* r = R + b * r_batch_stride + n * 9;
        const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
        unsigned c[4] = {(unsigned)j, (unsigned)b | ((unsigned)(t >> 32) << 16), kDiffuseTag, (unsigned)t};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        float z0, z1, z2, z3;
        box_muller4(c, z0, z1, z2, z3);
        w0 = sigma * z0; w1 = sigma * z1; w2 = sigma * z2;
        float a = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
        // The clip leaves 2^-21 of room on both sides of the comparison, so that the rounded vector's exact norm stays <= max_angle.
        if (max_angle > 0.0f && a * 1.00000048f > max_angle) {
            const float s = (max_angle / a) * 0.99999952f;
            w0 *= s; w1 *= s; w2 *= s;
            a = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
        }
        // q(w) = (cos a/2, sin(a/2) w / a); sin(a/2) / a -> 1/2 - a^2/48 as a -> 0
        float sh, ch;
        sincosf(0.5f * a, &sh, &ch);
        const float kq = a < 1e-3f ? 0.5f - a * a * (1.0f / 48.0f) : sh / a;
        const float dr = ch, di = kq * w0, dj = kq * w1, dk = kq * w2;
        // q(R) by Shepperd's branch: divide by the largest of the four components
        float qr, qi, qj, qk;
        const float tr = r00 + r11 + r22;
        if (tr > 0.0f) {
            const float s = 2.0f * sqrtf(tr + 1.0f);
            qr = 0.25f * s; qi = (r21 - r12) / s; qj = (r02 - r20) / s; qk = (r10 - r01) / s;
        } else if (r00 > r11 && r00 > r22) {
            const float s = 2.0f * sqrtf(1.0f + r00 - r11 - r22);
            qr = (r21 - r12) / s; qi = 0.25f * s; qj = (r01 + r10) / s; qk = (r02 + r20) / s;
        } else if (r11 > r22) {
            const float s = 2.0f * sqrtf(1.0f + r11 - r00 - r22);
            qr = (r02 - r20) / s; qi = (r01 + r10) / s; qj = 0.25f * s; qk = (r12 + r21) / s;
        } else {
            const float s = 2.0f * sqrtf(1.0f + r22 - r00 - r11);
            qr = (r10 - r01) / s; qi = (r02 + r20) / s; qj = (r12 + r21) / s; qk = 0.25f * s;
        }
        // Hamilton product q(R) q(w): the matrix of a product is the product of the matrices, R exp([w]x)
        float pr = qr * dr - qi * di - qj * dj - qk * dk;
        float pi = qr * di + qi * dr + qj * dk - qk * dj;
        float pj = qr * dj - qi * dk + qj * dr + qk * di;
        float pk = qr * dk + qi * dj - qj * di + qk * dr;
        const float inv = 1.0f / sqrtf(fmaxf(pr * pr + pi * pi + pj * pj + pk * pk, 1e-30f));
        pr *= inv; pi *= inv; pj *= inv; pk *= inv;
        quaternion_matrix(pr, pi, pj, pk, o);
    }
    if (omega) {
        float* w = omega + i * 3;
        w[0] = w0; w[1] = w1; w[2] = w2;
    }
}

// ---------------------------------------------------------------------------------
// Constant-velocity predict step (ahv_predict_rotations_f32, include/ahv.h): a particle is (R, v), v its body-frame rotation
// vector per frame.  One thread per slot (b, j), as diffuse_rotations_kernel; slot classes in this precedence:
//   elite  j == 0 with a key: R and v of row decode(key_b) copied bit for bit
//   coast  j == 1 with a key and `coast`: R_n exp([v_n]x), no noise -- the constant-velocity prediction of the previous arg-max
//   fresh  j >= M - n_fresh: the Haar rotation diffuse_rotations_kernel writes for the same (seed, step, b, j), v = 0
//   else   v' = damping v_i + sigma_vel y (clipped to max_speed), w = v' + sigma z (the second term clipped to max_angle),
//          out = R_i exp([w]x) composed as unit quaternions and normalised, exactly as diffuse_rotations_kernel does
// z is the block diffuse_rotations_kernel draws (third counter word kDiffuseTag), y a second block (kVelocityTag).
// The composition is compose_rotation_vector below, shared with smooth_step_kernel: the sequence of diffuse_rotations_kernel,
// which keeps its own copy on purpose -- that kernel's instructions are pinned, so nothing is factored out of it.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }  // false for NaN

// o = M(normalise(q(r) q(w))), the matrix of r exp([w]x), composed as unit quaternions and normalised.
__device__ __forceinline__ void compose_rotation_vector(const float (&r)[9], float w0, float w1, float w2, float* __restrict__ o)
{
    const float a = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
    // q(w) = (cos a/2, sin(a/2) w / a); sin(a/2) / a -> 1/2 - a^2/48 as a -> 0
    float sh, ch;
    sincosf(0.5f * a, &sh, &ch);
    const float kq = a < 1e-3f ? 0.5f - a * a * (1.0f / 48.0f) : sh / a;
    const float dr = ch, di = kq * w0, dj = kq * w1, dk = kq * w2;
    // q(R) by Shepperd's branch: divide by the largest of the four components
    float qr, qi, qj, qk;
    const float tr = r[0] + r[4] + r[8];
    if (tr > 0.0f) {
        const float s = 2.0f * sqrtf(tr + 1.0f);
        qr = 0.25f * s; qi = (r[7] - r[5]) / s; qj = (r[2] - r[6]) / s; qk = (r[3] - r[1]) / s;
    } else if (r[0] > r[4] && r[0] > r[8]) {
        const float s = 2.0f * sqrtf(1.0f + r[0] - r[4] - r[8]);
        qr = (r[7] - r[5]) / s; qi = 0.25f * s; qj = (r[1] + r[3]) / s; qk = (r[2] + r[6]) / s;
    } else if (r[4] > r[8]) {
        const float s = 2.0f * sqrtf(1.0f + r[4] - r[0] - r[8]);
        qr = (r[2] - r[6]) / s; qi = (r[1] + r[3]) / s; qj = 0.25f * s; qk = (r[5] + r[7]) / s;
    } else {
        const float s = 2.0f * sqrtf(1.0f + r[8] - r[0] - r[4]);
        qr = (r[3] - r[1]) / s; qi = (r[2] + r[6]) / s; qj = (r[5] + r[7]) / s; qk = 0.25f * s;
    }
    // Hamilton product q(R) q(w): the matrix of a product is the product of the matrices, R exp([w]x)
    float pr = qr * dr - qi * di - qj * dj - qk * dk;
    float pi = qr * di + qi * dr + qj * dk - qk * dj;
    float pj = qr * dj - qi * dk + qj * dr + qk * di;
    float pk = qr * dk + qi * dj - qj * di + qk * dr;
    const float inv = 1.0f / sqrtf(fmaxf(pr * pr + pi * pi + pj * pj + pk * pk, 1e-30f));
    pr *= inv; pi *= inv; pj *= inv; pk *= inv;
    quaternion_matrix(pr, pi, pj, pk, o);
}

constexpr unsigned kVelocityTag = 0x56454Cu;

// Scales (x, y, z) so that its norm is <= limit (limit > 0; 0 means no limit) and returns the norm of the result.  2^-21 of
// room on both sides of the comparison: the rounded vector's exact norm stays <= limit.  A NaN norm is left alone.
__device__ __forceinline__ float clip_norm(float& x, float& y, float& z, float limit)
{
    float a = sqrtf(x * x + y * y + z * z);
    if (limit > 0.0f && a * 1.00000048f > limit) {
        const float s = (limit / a) * 0.99999952f;
        x *= s; y *= s; z *= s;
        a = sqrtf(x * x + y * y + z * z);
    }
    return a;
}

__global__ __launch_bounds__(256) void predict_rotations_kernel(const long long* __restrict__ idx, const float* __restrict__ R,
                                                                long r_batch_stride, const float* __restrict__ V,
                                                                long v_batch_stride, long N, const key_t* __restrict__ best_key,
                                                                long M, long n_fresh, unsigned long long seed,
                                                                const long long* __restrict__ step, float sigma, float sigma_vel,
                                                                float damping, float max_angle, float max_speed, int coast,
                                                                float* __restrict__ out, float* __restrict__ vel_out,
                                                                float* __restrict__ omega)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const long b = blockIdx.y;
    const unsigned long long t = (unsigned long long)*step;
    const long i = b * M + j;
    float* o = out + i * 9;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    const bool elite = best_key && j == 0, coasting = best_key && j == 1 && coast;
    if (!elite && !coasting && j >= M - n_fresh) {
        haar_rotation(seed ^ kFreshSeed, (t * (unsigned long long)gridDim.y + (unsigned long long)b) * (unsigned long long)M + (unsigned long long)j, o);
    } else {
        long n;
        if (elite || coasting) {
            const key_t key = best_key[b];
            n = key_index(key);
            n = (key == kKeyEmpty || n < 0 || n >= N) ? 0 : n;  // as diffuse_rotations_kernel: stay in bounds
        } else {
            n = idx ? (long)idx[i] : j % N;
            n = (n < 0 || n >= N) ? 0 : n;
        }
        const float* r = R + b * r_batch_stride + n * 9;
        if (V) {
            const float* v = V + b * v_batch_stride + n * 3;
            v0 = v[0]; v1 = v[1]; v2 = v[2];
        }
        if (elite) {
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k] = r[k];
        } else {
            const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
            if (coasting) {
                w0 = v0; w1 = v1; w2 = v2;
            } else {
                const unsigned cb = (unsigned)b | ((unsigned)(t >> 32) << 16);
                unsigned c[4] = {(unsigned)j, cb, kVelocityTag, (unsigned)t};
                philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
                float y0, y1, y2, y3;
                box_muller4(c, y0, y1, y2, y3);
                v0 = fmaf(damping, v0, sigma_vel * y0); v1 = fmaf(damping, v1, sigma_vel * y1); v2 = fmaf(damping, v2, sigma_vel * y2);
                clip_norm(v0, v1, v2, max_speed);
                c[0] = (unsigned)j; c[1] = cb; c[2] = kDiffuseTag; c[3] = (unsigned)t;
                philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
                float z0, z1, z2, z3;
                box_muller4(c, z0, z1, z2, z3);
                float p0 = sigma * z0, p1 = sigma * z1, p2 = sigma * z2;
                clip_norm(p0, p1, p2, max_angle);
                w0 = v0 + p0; w1 = v1 + p1; w2 = v2 + p2;
            }
            const float rr[9] = {r00, r01, r02, r10, r11, r12, r20, r21, r22};
            compose_rotation_vector(rr, w0, w1, w2, o);
        }
    }
    float* vo = vel_out + i * 3;
    vo[0] = v0; vo[1] = v1; vo[2] = v2;
    if (omega) {
        float* w = omega + i * 3;
        w[0] = w0; w[1] = w1; w[2] = w2;
    }
}

// Start of a tracker step (ahv_track_advance): u[b] of step t + 1, then the counter itself.  One workgroup: the barrier
// orders every read of *step before the one write.
__global__ __launch_bounds__(256) void track_advance_kernel(unsigned long long seed, long long* step, int B, float* __restrict__ u)
{
    const unsigned long long t1 = (unsigned long long)*step + 1ull;
    for (int b = threadIdx.x; b < B; b += 256) {
        unsigned c[4] = {(unsigned)b, (unsigned)(t1 >> 32), kAdvanceTag, (unsigned)t1};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        u[b] = (float)(c[0] >> 8) * (1.0f / 16777216.0f);  // 24 bits: [0, 1)
    }
    __syncthreads();
    if (threadIdx.x == 0) *step = (long long)t1;
}

// ---------------------------------------------------------------------------------
// Trajectory smoothing over the particle history (ahv_smooth_step_f32 / ahv_smooth_backtrace_f32, include/ahv.h): a Viterbi
// recursion over the particle sets of the last H frames, kept in a ring the caller owns, and the backtrace.
//
// Step: a workgroup owns kSmoothSucc = 16 successors j of one sample and splits the predecessors 16 ways: lane l of wave w
// holds successor l mod 16 (the nine entries of R_j in registers) and belongs to group g = 4 w + l / 16.  The predecessors (the
// previous slot's predicted poses and deltas) go through LDS in tiles of 256 rows of 12 floats (nine entries, delta_i - m, two
// of padding: three 16-byte reads).  Thread k stages row k of a tile -- loaded into registers while the tile before is being
// walked -- and group g walks rows g, 16 + g, ..., 240 + g: the four groups of a wave read four adjacent rows, 192 contiguous
// bytes, so the reads of a 16-lane group broadcast and the four do not share a bank.  A group meets its rows in increasing i
// and keeps (max, first index); the 16 partial results of a successor are merged by (larger value, then lower index), four by
// lane shuffles and the waves' in LDS.  Every c_ij is one expression, evaluated once, and (max, lowest index) does not depend
// on the order: the bytes do not depend on the split.  At M = 4 096 that is 256 workgroups, one per CU, 256 pairs per lane.
// A row whose delta is not finite, and a row past the end of the set, is staged with NaN in place of delta_i - m: its c_ij is
// NaN, which no comparison selects, as is the c_ij of a NaN matrix.  The workgroup reads the previous slot only and writes its
// own rows of the current slot.
// ---------------------------------------------------------------------------------
constexpr int kSmoothSucc = 16, kSmoothTile = 256, kSmoothRow = 12;

// (value, index) merge of the Viterbi maximum: the larger value, then the lower index.
__device__ __forceinline__ void merge_first_max(float& v, int& i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(256) void smooth_step_kernel(const float* __restrict__ R_cur, const float* __restrict__ scores,
                                                          const float* __restrict__ V_cur, const long long* __restrict__ step,
                                                          long long first_step, int M, long long H, float beta, float inv4s2,
                                                          float jump, float damping, float* __restrict__ hist_R,
                                                          float* __restrict__ hist_P, float* __restrict__ hist_delta,
                                                          int* __restrict__ hist_back)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_v[4][kSmoothSucc];
    __shared__ int part_i[4][kSmoothSucc];
    __shared__ float wave_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int succ = lane & (kSmoothSucc - 1), group = 4 * wave + (lane >> 4);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long t = *step;
    const long slot = (long)(((t % H) + H) % H), prev = (long)((((t - 1) % H) + H) % H);  // int64: t may be past 2^32
    const long row_cur = (slot * nb + b) * (long)M, row_prev = (prev * nb + b) * (long)M;
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = R_cur + (b * (long)M + j) * 9;

    // hist_R[slot]: this workgroup's rows, bit for bit
    if (tid < rows * 9) hist_R[(row_cur + j0) * 9 + tid] = R_cur[(b * (long)M + j0) * 9 + tid];
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];

    // m: the largest finite delta of the previous slot (every workgroup of the sample finds the same one)
    bool has_prev = t > first_step;
    float m = -__builtin_inff();
    if (has_prev) {
        for (long i = tid; i < M; i += 256) {
            const float d = hist_delta[row_prev + i];
            if (finite_f(d)) m = fmaxf(m, d);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
        if (lane == 0) wave_max[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
        has_prev = finite_f(m);
    }

    float best = -__builtin_inff();
    int best_i = -1;
    if (has_prev) {
        const float neg_jump = -jump;
        const float* P = hist_P ? hist_P : hist_R;
        // this thread's row of a tile: nine entries and delta_i - m, NaN for a dead row and past the end
        float stage[10];
        const auto load_row = [&](long i) {
#pragma unroll
            for (int k = 0; k < 9; ++k) stage[k] = 0.0f;
            stage[9] = __builtin_nanf("");
            if (i < M) {
                const float* src = P + (row_prev + i) * 9;
#pragma unroll
                for (int k = 0; k < 9; ++k) stage[k] = src[k];
                const float v = hist_delta[row_prev + i];
                if (finite_f(v)) stage[9] = v - m;
            }
        };
        load_row(tid);
        for (long i0 = 0; i0 < M; i0 += kSmoothTile) {
            __syncthreads();  // the previous tile has been read by every wave
            f32x4* dst = reinterpret_cast<f32x4*>(tile + tid * kSmoothRow);
            dst[0] = f32x4{stage[0], stage[1], stage[2], stage[3]};
            dst[1] = f32x4{stage[4], stage[5], stage[6], stage[7]};
            dst[2] = f32x4{stage[8], stage[9], 0.0f, 0.0f};
            __syncthreads();
            if (i0 + kSmoothTile < M) load_row(i0 + kSmoothTile + tid);  // in flight while this tile is walked
#pragma unroll 4
            for (int p = 0; p < kSmoothTile / 16; ++p) {
                const int row = 16 * p + group;
                const f32x4 a = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow);
                const f32x4 c = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 4);
                const f32x4 d = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 8);
                // ||P_i - R_j||_F^2 from the nine differences (3 - tr cancels for the near pairs that decide the maximum)
                const float e0 = a[0] - r[0], e1 = a[1] - r[1], e2 = a[2] - r[2], e3 = a[3] - r[3], e4 = c[0] - r[4];
                const float e5 = c[1] - r[5], e6 = c[2] - r[6], e7 = c[3] - r[7], e8 = d[0] - r[8];
                float q = e0 * e0;
                q = fmaf(e1, e1, q); q = fmaf(e2, e2, q); q = fmaf(e3, e3, q); q = fmaf(e4, e4, q);
                q = fmaf(e5, e5, q); q = fmaf(e6, e6, q); q = fmaf(e7, e7, q); q = fmaf(e8, e8, q);
                const float w = -(q * inv4s2);
                const float cij = d[1] + (w < neg_jump ? neg_jump : w);  // (a NaN w stays NaN: fmaxf would drop it)
                if (cij > best) { best = cij; best_i = (int)i0 + row; }
            }
        }
        // the four groups of a wave (lanes succ, succ + 16, + 32, + 48), then the four waves
#pragma unroll
        for (int s = 16; s <= 32; s <<= 1) merge_first_max(best, best_i, __shfl_xor(best, s, 64), __shfl_xor(best_i, s, 64));
        if (lane < kSmoothSucc) { part_v[wave][lane] = best; part_i[wave][lane] = best_i; }
        __syncthreads();
    }

    if (tid < kSmoothSucc && live) {
        if (has_prev) {
#pragma unroll
            for (int w = 1; w < 4; ++w) merge_first_max(best, best_i, part_v[w][lane], part_i[w][lane]);
        }
        const float s = scores[b * (long)M + j];
        float delta = -__builtin_inff();
        int back = -1;
        if (finite_f(s)) {
            delta = beta * s;
            if (best_i >= 0) { delta += best; back = best_i; }
        }
        hist_delta[row_cur + j] = delta;
        hist_back[row_cur + j] = back;
    }
    if (hist_P && wave == 1 && lane < kSmoothSucc && live) {
        const float* v = V_cur + (b * (long)M + j) * 3;
        compose_rotation_vector(r, damping * v[0], damping * v[1], damping * v[2], hist_P + (row_cur + j) * 9);
    }
}

// Backtrace: one workgroup per sample walks t, t - 1, ... over F <= H frames and writes the outputs oldest first.  The index
// carried to the frame before is back[j]; with none carried (the start, or behind a break) the frame's first arg-max over its
// finite deltas is taken by the whole workgroup.  `carry` is the same in every thread, so the barriers are uniform.
__global__ __launch_bounds__(256) void smooth_backtrace_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_delta,
                                                               const int* __restrict__ hist_back, const long long* __restrict__ step,
                                                               long long first_step, int M, long long H, int F,
                                                               long long* __restrict__ path_idx, float* __restrict__ path_R)
{
    __shared__ float part_v[4];
    __shared__ int part_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x, nb = gridDim.x;
    const long long t = *step;
    int carry = -1;
    for (int k = 0; k < F; ++k) {
        const long long tk = t - k;
        const long o = b * (long)F + (F - 1 - k);
        long row = 0;
        if (tk < first_step) {
            carry = -1;  // never recorded
        } else {
            row = ((long)(((tk % H) + H) % H) * nb + b) * (long)M;
            if (carry < 0) {
                float v = -__builtin_inff();
                int vi = -1;
                for (long i = tid; i < M; i += 256) {
                    const float d = hist_delta[row + i];
                    if (finite_f(d) && (vi < 0 || d > v)) { v = d; vi = (int)i; }
                }
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) {
                    const float ov = __shfl_xor(v, s, 64);
                    const int oi = __shfl_xor(vi, s, 64);
                    if (oi >= 0 && (vi < 0 || ov > v || (ov == v && oi < vi))) { v = ov; vi = oi; }
                }
                if (lane == 0) { part_v[wave] = v; part_i[wave] = vi; }
                __syncthreads();
                v = part_v[0]; vi = part_i[0];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const float ov = part_v[w];
                    const int oi = part_i[w];
                    if (oi >= 0 && (vi < 0 || ov > v || (ov == v && oi < vi))) { v = ov; vi = oi; }
                }
                __syncthreads();  // part_* are free for the next break
                carry = vi;
            }
        }
        if (tid == 0) path_idx[o] = carry;
        if (tid < 9) path_R[o * 9 + tid] = carry >= 0 ? hist_R[(row + carry) * 9 + tid] : (tid % 4 == 0 ? 1.0f : 0.0f);
        if (carry >= 0) {
            const int nxt = hist_back[row + carry];
            carry = (nxt >= 0 && nxt < M) ? nxt : -1;  // a ring the step did not write: stay in bounds
        }
    }
}

// ---------------------------------------------------------------------------------
// Marginal smoothing over the same ring (ahv_marginal_step_f32 / ahv_marginal_smooth_f32, include/ahv.h): the sum-product
// recursions of the hidden-Markov model whose max-product recursion is smooth_step_kernel -- the same transition, the same
// decomposition, log-sum-exp in place of max.  marginal_walk is the one pairwise pass of both directions: a workgroup owns
// kSmoothSucc "owner" rows of one sample (nine entries in registers) and the "other" rows go through LDS in the tiles of
// smooth_step_kernel, the tenth float of a row being the other row's log-weight minus the largest finite one, NaN for a dead
// row and past the end.  A lane keeps a running (max, sum) pair over the rows of its group, met in increasing
// index; a candidate that is NaN or -inf is skipped explicitly (expf(NaN) would poison the sum, where the Viterbi compare
// never selected it).  The pairs merge as (max, sum) pairs in a fixed order: lanes 16 apart, lanes 32 apart, then waves 1, 2, 3
// onto wave 0 in LDS.  The running maximum is the data's own, not a fixed offset: with jump = +inf and far clusters every
// term may sit near -365 and still sum to a finite value.  Bitwise reproducible and independent of B; NOT independent of the
// split (a sum, unlike a max, depends on the order), so the 16 x 16 split of the rows is part of the contract.
//   forward   owners R_cur, others P/R and alpha of the previous slot: alpha_j = a_j + LSE_i[(alpha_i - m) + w_ij]
//   backward  owners P/R of slot tau, others R and g = emit + beta of slot tau + 1: beta_i = LSE_j[w_ij + (g_j - m')]
// ---------------------------------------------------------------------------------
// One more term of a running log-sum-exp, sum = sum_k exp(x_k - mx), from (-inf, 0).  x is finite: the caller skips NaN and -inf.
__device__ __forceinline__ void lse_add(float& mx, float& sum, float x)
{
    const float d = x - mx;  // +inf at the first term: e = 0, sum = 1
    const float e = expf(-fabsf(d));
    sum = d > 0.0f ? fmaf(sum, e, 1.0f) : sum + e;
    mx = fmaxf(mx, x);
}

// (max, sum) merge; an empty side is (-inf, 0).
__device__ __forceinline__ void lse_merge(float& mx, float& sum, float omx, float osum)
{
    const float nm = fmaxf(mx, omx);
    if (nm > -__builtin_inff()) {
        sum = sum * expf(mx - nm) + osum * expf(omx - nm);
        mx = nm;
    }
}

// The pairwise pass.  r: the owner row of this lane; other: the other slot's rows (nine floats each); the log-weight of other
// row i is lw_a[i] + (lw_b ? lw_b[i] : 0), alive iff finite.  Returns whether any other row is alive (uniform over the
// workgroup); then threads 0..15 hold the merged (mx, sum) of their owner, sum == 0 when no edge reaches it.
__device__ __forceinline__ bool marginal_walk(const float (&r)[9], const float* __restrict__ other, const float* __restrict__ lw_a,
                                              const float* __restrict__ lw_b, int M, float inv4s2, float jump, float* tile,
                                              float (*part_m)[kSmoothSucc], float (*part_s)[kSmoothSucc], float* wave_max,
                                              float& mx, float& sum)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int group = 4 * wave + (lane >> 4);
    float m = -__builtin_inff();
    for (long i = tid; i < M; i += 256) {
        const float d = lw_a[i] + (lw_b ? lw_b[i] : 0.0f);
        if (finite_f(d)) m = fmaxf(m, d);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    mx = -__builtin_inff();
    sum = 0.0f;
    if (!finite_f(m)) return false;

    const float neg_jump = -jump;
    float stage[10];
    const auto load_row = [&](long i) {
#pragma unroll
        for (int k = 0; k < 9; ++k) stage[k] = 0.0f;
        stage[9] = __builtin_nanf("");
        if (i < M) {
            const float* src = other + i * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) stage[k] = src[k];
            const float v = lw_a[i] + (lw_b ? lw_b[i] : 0.0f);
            if (finite_f(v)) stage[9] = v - m;
        }
    };
    load_row(tid);
    for (long i0 = 0; i0 < M; i0 += kSmoothTile) {
        __syncthreads();  // the previous tile has been read by every wave
        f32x4* dst = reinterpret_cast<f32x4*>(tile + tid * kSmoothRow);
        dst[0] = f32x4{stage[0], stage[1], stage[2], stage[3]};
        dst[1] = f32x4{stage[4], stage[5], stage[6], stage[7]};
        dst[2] = f32x4{stage[8], stage[9], 0.0f, 0.0f};
        __syncthreads();
        if (i0 + kSmoothTile < M) load_row(i0 + kSmoothTile + tid);  // in flight while this tile is walked
#pragma unroll 4
        for (int p = 0; p < kSmoothTile / 16; ++p) {
            const int row = 16 * p + group;
            const f32x4 a = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow);
            const f32x4 c = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 4);
            const f32x4 d = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 8);
            const float e0 = a[0] - r[0], e1 = a[1] - r[1], e2 = a[2] - r[2], e3 = a[3] - r[3], e4 = c[0] - r[4];
            const float e5 = c[1] - r[5], e6 = c[2] - r[6], e7 = c[3] - r[7], e8 = d[0] - r[8];
            float q = e0 * e0;
            q = fmaf(e1, e1, q); q = fmaf(e2, e2, q); q = fmaf(e3, e3, q); q = fmaf(e4, e4, q);
            q = fmaf(e5, e5, q); q = fmaf(e6, e6, q); q = fmaf(e7, e7, q); q = fmaf(e8, e8, q);
            const float w = -(q * inv4s2);
            const float x = d[1] + (w < neg_jump ? neg_jump : w);  // NaN for a dead row, a row past the end and a NaN matrix
            if (x > -__builtin_inff()) lse_add(mx, sum, x);        // (false for NaN)
        }
    }
    // the four groups of a wave (lanes succ, succ + 16, + 32, + 48), then the four waves
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1) {
        const float om = __shfl_xor(mx, s, 64), os = __shfl_xor(sum, s, 64);
        // both lanes of a pair must compute the same bytes: the lower lane's pair first
        if (lane & s) { float tm = om, ts = os; lse_merge(tm, ts, mx, sum); mx = tm; sum = ts; }
        else lse_merge(mx, sum, om, os);
    }
    if (lane < kSmoothSucc) { part_m[wave][lane] = mx; part_s[wave][lane] = sum; }
    __syncthreads();
    if (tid < kSmoothSucc) {
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(mx, sum, part_m[w][lane], part_s[w][lane]);
    }
    return true;
}

// Forward step: alpha and emit of slot t mod H from the previous slot.  Reads hist_R / hist_P of slot t - 1 only.
__global__ __launch_bounds__(256) void marginal_step_kernel(const float* __restrict__ R_cur, const float* __restrict__ scores,
                                                            const long long* __restrict__ step, long long first_step, int M,
                                                            long long H, float beta, float inv4s2, float jump,
                                                            const float* __restrict__ hist_R, const float* __restrict__ hist_P,
                                                            float* __restrict__ hist_alpha, float* __restrict__ hist_emit)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_m[4][kSmoothSucc], part_s[4][kSmoothSucc], wave_max[4];
    const int tid = threadIdx.x, succ = tid & (kSmoothSucc - 1);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long t = *step;
    const long slot = (long)(((t % H) + H) % H), prev = (long)((((t - 1) % H) + H) % H);
    const long row_cur = (slot * nb + b) * (long)M, row_prev = (prev * nb + b) * (long)M;
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = R_cur + (b * (long)M + j) * 9;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];
    float mx = -__builtin_inff(), sum = 0.0f;
    bool has_prev = t > first_step;
    if (has_prev)
        has_prev = marginal_walk(r, (hist_P ? hist_P : hist_R) + row_prev * 9, hist_alpha + row_prev, nullptr, M, inv4s2, jump, tile,
                                 part_m, part_s, wave_max, mx, sum);
    if (tid < kSmoothSucc && live) {
        const float s = scores[b * (long)M + j];
        float emit = -__builtin_inff(), alpha = -__builtin_inff();
        if (finite_f(s)) {
            emit = beta * s;
            if (!has_prev) alpha = emit;
            else if (sum > 0.0f) alpha = emit + (mx + logf(sum));
        }
        hist_alpha[row_cur + j] = alpha;
        hist_emit[row_cur + j] = emit;
    }
}

// Backward step for frame tau = t - back, output column f = F - 1 - back: beta(tau) into logw[b][f] from slot tau + 1, whose
// beta is logw[b][f + 1] (zero for the newest frame, back == 1).  A frame before first_step is left to the finish kernel.
__global__ __launch_bounds__(256) void marginal_backward_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_P,
                                                                const float* __restrict__ hist_emit,
                                                                const long long* __restrict__ step, long long first_step, int M,
                                                                long long H, int F, int back, float inv4s2, float jump,
                                                                float* __restrict__ logw)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_m[4][kSmoothSucc], part_s[4][kSmoothSucc], wave_max[4];
    const int tid = threadIdx.x, succ = tid & (kSmoothSucc - 1);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long tau = *step - back;
    if (tau < first_step) return;  // the whole workgroup
    const long slot = (long)(((tau % H) + H) % H), next = (long)((((tau + 1) % H) + H) % H);
    const long row_own = (slot * nb + b) * (long)M, row_next = (next * nb + b) * (long)M;
    const int f = F - 1 - back;
    float* out = logw + (b * (long)F + f) * (long)M;
    const float* beta_next = back == 1 ? nullptr : out + M;
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = (hist_P ? hist_P : hist_R) + (row_own + j) * 9;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];
    float mx, sum;
    const bool has_next = marginal_walk(r, hist_R + row_next * 9, hist_emit + row_next, beta_next, M, inv4s2, jump, tile, part_m,
                                        part_s, wave_max, mx, sum);
    if (tid < kSmoothSucc && live) out[j] = !has_next ? 0.0f : (sum > 0.0f ? mx + logf(sum) : -__builtin_inff());
}

// Finish: one workgroup per (sample, frame).  x_i = alpha_i + beta_i (beta = 0 in the newest frame), log gamma_i = x_i - LSE x
// written over beta, the first arg-max of the written values and its pose.  Thread k sums rows k, k + 256, ... in increasing
// order; the pairs merge lane by lane (xor 1, 2, ..., 32, the lower lane's pair first) and then wave by wave.
__global__ __launch_bounds__(256) void marginal_finish_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_alpha,
                                                              const long long* __restrict__ step, long long first_step, int M,
                                                              long long H, int F, float* __restrict__ logw,
                                                              long long* __restrict__ out_idx, float* __restrict__ out_R)
{
    __shared__ float part_m[4], part_s[4];
    __shared__ int part_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    const long b = blockIdx.y, nb = gridDim.y;
    const long long tau = *step - (F - 1 - f);
    const long o = b * (long)F + f;
    float* lw = logw + o * (long)M;
    const bool newest = f == F - 1;
    const float ninf = -__builtin_inff();
    long row = 0;
    int best_i = -1;
    if (tau >= first_step) {
        row = ((long)(((tau % H) + H) % H) * nb + b) * (long)M;
        float mx = ninf, sum = 0.0f;
        for (long i = tid; i < M; i += 256) {
            const float x = hist_alpha[row + i] + (newest ? 0.0f : lw[i]);
            if (finite_f(x)) lse_add(mx, sum, x);
        }
#pragma unroll
        for (int s = 1; s <= 32; s <<= 1) {
            const float om = __shfl_xor(mx, s, 64), os = __shfl_xor(sum, s, 64);
            if (lane & s) { float tm = om, ts = os; lse_merge(tm, ts, mx, sum); mx = tm; sum = ts; }
            else lse_merge(mx, sum, om, os);
        }
        if (lane == 0) { part_m[wave] = mx; part_s[wave] = sum; }
        __syncthreads();
        mx = part_m[0]; sum = part_s[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(mx, sum, part_m[w], part_s[w]);
        __syncthreads();  // part_m is reused below
        if (sum > 0.0f) {
            const float log_z = mx + logf(sum);
            float best = ninf;
            for (long i = tid; i < M; i += 256) {
                const float x = hist_alpha[row + i] + (newest ? 0.0f : lw[i]);
                const float g = finite_f(x) ? x - log_z : ninf;
                lw[i] = g;
                if (g > best) { best = g; best_i = (int)i; }  // increasing i: the first one of this thread
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const float ov = __shfl_xor(best, s, 64);
                const int oi = __shfl_xor(best_i, s, 64);
                if (oi >= 0 && (best_i < 0 || ov > best || (ov == best && oi < best_i))) { best = ov; best_i = oi; }
            }
            if (lane == 0) { part_m[wave] = best; part_i[wave] = best_i; }
            __syncthreads();
            best = part_m[0]; best_i = part_i[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float ov = part_m[w];
                const int oi = part_i[w];
                if (oi >= 0 && (best_i < 0 || ov > best || (ov == best && oi < best_i))) { best = ov; best_i = oi; }
            }
        }
    }
    if (best_i < 0)
        for (long i = tid; i < M; i += 256) lw[i] = ninf;
    if (tid == 0) out_idx[o] = best_i;
    if (tid < 9) out_R[o * 9 + tid] = best_i >= 0 ? hist_R[(row + best_i) * 9 + tid] : (tid % 4 == 0 ? 1.0f : 0.0f);
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

hipError_t launch_random_rotations(uint64_t seed, uint64_t offset, int64_t N, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(random_rotations_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream,
                       (unsigned long long)seed, (unsigned long long)offset, (long)N, out);
    return hipGetLastError();
}

hipError_t launch_diffuse_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const int64_t* best_key,
                                    int64_t M, int64_t n_fresh, int B, uint64_t seed, const int64_t* step, float sigma,
                                    float max_angle, float* out, float* omega, hipStream_t stream)
{
    hipLaunchKernelGGL(diffuse_rotations_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                       reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, (long)N,
                       reinterpret_cast<const key_t*>(best_key), (long)M, (long)n_fresh, (unsigned long long)seed,
                       reinterpret_cast<const long long*>(step), sigma, max_angle, out, omega);
    return hipGetLastError();
}

hipError_t launch_predict_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V,
                                    int64_t v_batch_stride, int64_t N, const int64_t* best_key, int64_t M, int64_t n_fresh, int B,
                                    uint64_t seed, const int64_t* step, float sigma, float sigma_vel, float damping,
                                    float max_angle, float max_speed, int coast, float* out, float* vel_out, float* omega,
                                    hipStream_t stream)
{
    hipLaunchKernelGGL(predict_rotations_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                       reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, V, (long)v_batch_stride, (long)N,
                       reinterpret_cast<const key_t*>(best_key), (long)M, (long)n_fresh, (unsigned long long)seed,
                       reinterpret_cast<const long long*>(step), sigma, sigma_vel, damping, max_angle, max_speed, coast, out,
                       vel_out, omega);
    return hipGetLastError();
}

hipError_t launch_track_advance(uint64_t seed, int64_t* step, int B, float* u, hipStream_t stream)
{
    hipLaunchKernelGGL(track_advance_kernel, dim3(1), dim3(256), 0, stream, (unsigned long long)seed,
                       reinterpret_cast<long long*>(step), B, u);
    return hipGetLastError();
}

hipError_t launch_smooth_step(const float* R_cur, const float* scores, const float* V_cur, const int64_t* step, int64_t first_step,
                              int B, int64_t M, int64_t H, float beta, float inv4s2, float jump, float damping, float* hist_R,
                              float* hist_P, float* hist_delta, int32_t* hist_back, hipStream_t stream)
{
    hipLaunchKernelGGL(smooth_step_kernel, dim3((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B), dim3(256), 0, stream,
                       R_cur, scores, V_cur, reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H,
                       beta, inv4s2, jump, damping, hist_R, hist_P, hist_delta, reinterpret_cast<int*>(hist_back));
    return hipGetLastError();
}

hipError_t launch_smooth_backtrace(const float* hist_R, const float* hist_delta, const int32_t* hist_back, const int64_t* step,
                                   int64_t first_step, int B, int64_t M, int64_t H, int64_t F, int64_t* path_idx, float* path_R,
                                   hipStream_t stream)
{
    hipLaunchKernelGGL(smooth_backtrace_kernel, dim3((unsigned)B), dim3(256), 0, stream, hist_R, hist_delta,
                       reinterpret_cast<const int*>(hist_back), reinterpret_cast<const long long*>(step), (long long)first_step,
                       (int)M, (long long)H, (int)F, reinterpret_cast<long long*>(path_idx), path_R);
    return hipGetLastError();
}

hipError_t launch_marginal_step(const float* R_cur, const float* scores, const int64_t* step, int64_t first_step, int B, int64_t M,
                                int64_t H, float beta, float inv4s2, float jump, const float* hist_R, const float* hist_P,
                                float* hist_alpha, float* hist_emit, hipStream_t stream)
{
    hipLaunchKernelGGL(marginal_step_kernel, dim3((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B), dim3(256), 0, stream,
                       R_cur, scores, reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, beta,
                       inv4s2, jump, hist_R, hist_P, hist_alpha, hist_emit);
    return hipGetLastError();
}

// F - 1 backward launches (frames t - 1, t - 2, ...: each reads the beta the launch before wrote) and the finish, in stream
// order: a linear chain under capture.
hipError_t launch_marginal_smooth(const float* hist_R, const float* hist_P, const float* hist_alpha, const float* hist_emit,
                                  const int64_t* step, int64_t first_step, int B, int64_t M, int64_t H, int64_t F, float inv4s2,
                                  float jump, float* logw, int64_t* idx, float* R, hipStream_t stream)
{
    const dim3 grid((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B);
    for (int64_t back = 1; back < F; ++back) {
        hipLaunchKernelGGL(marginal_backward_kernel, grid, dim3(256), 0, stream, hist_R, hist_P, hist_emit,
                           reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, (int)F, (int)back,
                           inv4s2, jump, logw);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(marginal_finish_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, stream, hist_R, hist_alpha,
                       reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, (int)F, logw,
                       reinterpret_cast<long long*>(idx), R);
    return hipGetLastError();
}

hipError_t launch_so3_grid(int64_t n_total, int64_t offset, int64_t N, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(so3_grid_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (long)n_total,
                       (long)offset, (long)N, out);
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

}  // namespace ahv
