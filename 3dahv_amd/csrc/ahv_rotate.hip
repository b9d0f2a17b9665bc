// ahv_rotate.hip -- the op-level rotate_volume: the tensor utils.rotate_volume returns (utils.py:113-131) and its adjoint
// w.r.t. the volume.  Three kernels: the (16,8,8,8) shared-volume forward, the generic forward, the volume adjoint.  The
// gradient w.r.t. the rotations (rotate_volume_rotation_grad_*_kernel) is in ahv_rotgrad.hip, next to
// score_rotation_grad_kernel whose gather it reuses: those kernels need that file's build flags (no SLP vectoriser: it
// un-contracts FMAs of the generic gradient), these were tuned under the default ones.  The trilinear rule all of them
// share is ahv_trilinear.h.
#include "ahv_device.h"
#include "ahv_launch.h"
#include "ahv_dual.h"
#include "ahv_exact.h"
#include "ahv_trilinear.h"

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
    if (stage_src_volume_scan(srcT, vol, tid, kRotThreads)) nf = 1u;
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
// What the generic forward and the adjoint share per output voxel: the centre, g = R p, and per axis the two rows' weights,
// clamped indices (stride 1: the row-major offset is formed per corner) and in-range flags.  Declarations in the kernel's
// scope, not a function filling a struct: that form changed both kernels' instruction sequences, this one does not.
#define AHV_GENERIC_AXES(v, r)                                                                                         \
    const TriVoxel p = tri_voxel(v, D, H, W, r);                                                                       \
    TriAxis<long> ax, ay, az;                                                                                          \
    tri_axis(tri_index(p.gx, W), W, 1L, ax);                                                                           \
    tri_axis(tri_index(p.gy, H), H, 1L, ay);                                                                           \
    tri_axis(tri_index(p.gz, D), D, 1L, az);                                                                           \
    const float wx[2] = {ax.w0, ax.w1}, wy[2] = {ay.w0, ay.w1}, wz[2] = {az.w0, az.w1};                                \
    const long ox[2] = {ax.o0, ax.o1}, oy[2] = {ay.o0, ay.o1}, oz[2] = {az.o0, az.o1};                                 \
    const bool ix[2] = {ax.d0 != 0.0f, ax.d1 != 0.0f}, iy[2] = {ay.d0 != 0.0f, ay.d1 != 0.0f}, iz[2] = {az.d0 != 0.0f, az.d1 != 0.0f}

__global__ __launch_bounds__(256) void rotate_volume_generic_kernel(
    const float* __restrict__ vol, long vol_batch_stride, const float* __restrict__ R, long N, int C, int D,
    int H, int W, float* __restrict__ out)
{
    const long plane = (long)D * H * W;
    const long total = N * plane;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / plane;
        const long v = i - n * plane;
        AHV_GENERIC_AXES(v, R + n * 9);
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
// unmodified reference scripts; the training path proper is the fused backward (ahv_backward.hip, ahv_bwd_volume.hip).
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
        AHV_GENERIC_AXES(v, R + n * 9);
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

#undef AHV_GENERIC_AXES

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

}  // namespace ahv
