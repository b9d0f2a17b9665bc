// ahv_rotgrad.hip -- the gradients w.r.t. the rotations: d score / d R of the fused scorer (score_rotation_grad_kernel) and
// d rotate_volume / d R of the op-level rotate_volume (rotate_volume_rotation_grad_*_kernel; its forward and volume adjoint
// are ahv_rotate.hip).  One family: nine sums per hypothesis, one workgroup per hypothesis, the trilinear rule of
// ahv_trilinear.h, bitwise reproducible.  Built without the SLP vectoriser, like the rest of the backward (Makefile): it
// un-contracts FMAs of the generic gradient.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ahv_bwd.h"
#include "ahv_launch.h"
#include "ahv_trilinear.h"

namespace ahv {

// ---------------------------------------------------------------------------------------------------
// d score / d R (ahv_score_rotation_grad_f32): kernel 2b (ahv_bwd_volume.hip) with its hard part removed.  The head pass
// (ACCUM = false, ahv_backward.hip: launch_score_backward_head_du) leaves du
// of every hypothesis in the workspace; here a TEAM of four waves -- one workgroup, wave m = channels 4 m .. 4 m + 3, the
// split and the W1^T fragments of kernel 2b -- forms dX = W1^T du half a volume at a time (rmw_dx_half: 192 fp32 MFMAs per
// wave and hypothesis) and, instead of scattering it, READS the eight corners of every rotated voxel from the channel-last
// source image in LDS:
//   s_corner = <dX[4 m .., p], V[4 m .., corner]>,   t_a(p) = sum_corners s_corner * d w_corner / d i_a,
//   d score / d R[a][b] = sum_p t_a(p) * 4 p_b        (i_a = 4 q_a + 3.5, q = R p: d i_a / d R[a][b] = 4 p_b)
// with grid_sampler_3d_backward's conventions: floor(i) is the cell (at an integer coordinate the derivative is
// V[i + 1] - V[i]) and a corner outside [0, 7]^3 contributes neither value nor derivative.
// One workgroup per hypothesis at a time, always: the nine sums of a hypothesis are formed by the same four waves in the
// same order whatever B, N, the grid or the cut into calls are -- lane sums over its 8 voxels (half 0 then half 1, plane
// order), a xor butterfly inside the wave, (w0 + w1) + (w2 + w3) across the team -- so grad_R is bitwise reproducible,
// and a launch of a single hypothesis still has four waves (and B * N workgroups spread over the chip).
// A sample whose volume, or a launch whose head weights, hold a NaN / inf reports NaN for its hypotheses (the project's
// rule for non-finite inputs, ahv_exact.h), found while the volume is staged; a hypothesis whose R holds one reports NaN too.
// ---------------------------------------------------------------------------------------------------
constexpr int kRotGradThreads = 256;

// the lane's four voxels of half volume H: plane al = 0..3 (depth 2 H + (al & 1) + 4 (al >> 1)), y = lane >> 3, x = lane & 7
template <int H>
__device__ __forceinline__ void rg_gather_half(float (&sum)[9], const float* xbuf, const float* src_ch, const float* Rm, int lane)
{
    const int yb = lane >> 3, xe = lane & 7;
    const float x4 = (float)xe - 3.5f, y4 = (float)yb - 3.5f;   // 4 * voxel-centre coordinate
#pragma unroll
    for (int al = 0; al < 4; ++al) {
        const float z4 = (float)(2 * H + (al & 1) + 4 * (al >> 1)) - 3.5f;
        const float* xp = xbuf + al * kXPlane + yb * kXRow + xe * 4;   // 8-byte aligned
        const f32x2 dlo = *reinterpret_cast<const f32x2*>(xp), dhi = *reinterpret_cast<const f32x2*>(xp + 2);
        rot_grad_voxel(sum, dlo[0], dlo[1], dhi[0], dhi[1], src_ch, Rm, x4, y4, z4);
    }
}

__global__ __launch_bounds__(kRotGradThreads) void score_rotation_grad_kernel(
    const float* __restrict__ vol_src, const float* __restrict__ R, long r_batch_stride, const float* __restrict__ W1,
    const float* __restrict__ W2, const float* __restrict__ b2, int B, long N, const float* __restrict__ du_ws,
    float* __restrict__ grad_R)
{
    __shared__ __attribute__((aligned(16))) float lds_src[kSrcFloats];
    __shared__ __attribute__((aligned(16))) float lds_x[4 * kXbufWords];   // per wave: dX of its 4 channels, half a volume
    __shared__ float lds_red[4 * 12];
    __shared__ unsigned lds_bad[2];   // [0]: a head weight is non-finite, [1]: the staged volume is
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xbuf = lds_x + m * kXbufWords;
    const float* src_ch = lds_src + 4 * m;
    if (tid < 2) lds_bad[tid] = 0u;
    __syncthreads();
    {
        bool bad = false;
        for (int i = tid; i < 32 * 384; i += kRotGradThreads) bad = bad || __builtin_amdgcn_classf(W1[i], 0x207);
        for (int i = tid; i < 32 * 32; i += kRotGradThreads) bad = bad || __builtin_amdgcn_classf(W2[i], 0x207);
        if (tid < 32) bad = bad || __builtin_amdgcn_classf(b2[tid], 0x207);
        if (bad) lds_bad[0] = 1u;
    }
    W1tFrags w1t;   // of channels 4 m .. 4 m + 3
    load_w1t_frags(w1t, W1, m, lane);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        __syncthreads();
        if (tid == 0) lds_bad[1] = 0u;
        __syncthreads();
        if (stage_src_volume_scan(lds_src, vol_src + (long)b * (16 * 512), tid, kRotGradThreads)) lds_bad[1] = 1u;
        __syncthreads();
        const bool poisoned = (lds_bad[0] | lds_bad[1]) != 0u;
        const float* Rb = R + (long)b * r_batch_stride;
        for (long h = blockIdx.x; h < N; h += gridDim.x) {
            float Rm[9];
            bool bad_r;
            load_rotation(Rm, bad_r, Rb + h * 9);
            DuRegs du;
            load_du_regs(du, du_ws + ((long)b * N + h) * 2048, lane);
            float sum[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) sum[i] = 0.0f;
            rmw_dx_half<0>(w1t, du, xbuf, lane);
            wave_lds_fence();
            rg_gather_half<0>(sum, xbuf, src_ch, Rm, lane);
            wave_lds_fence();
            rmw_dx_half<1>(w1t, du, xbuf, lane);
            wave_lds_fence();
            rg_gather_half<1>(sum, xbuf, src_ch, Rm, lane);
            wave_lds_fence();
            reduce_store_nine(sum, lds_red, tid, poisoned || bad_r, grad_R + ((long)b * N + h) * 9);
        }
    }
}

hipError_t launch_score_rotation_grad(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                      const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                      const float* grad_scores, float* du_ws, float* grad_R, int num_cu, hipStream_t stream)
{
    if (B == 0 || N == 0) return hipSuccess;
    const int gy = B < num_cu ? B : num_cu;
    // head pass: one wave per hypothesis; a short list is spread one hypothesis per workgroup over the chip
    hipError_t e = launch_score_backward_head_du(vol_src, feat_tgt, R, r_batch_stride, W1, W2, b2, B, N, grad_scores, du_ws, num_cu,
                                                 stream);
    if (e != hipSuccess) return e;
    {   // a team (= workgroup) per hypothesis, two workgroups fit a CU
        int64_t gx = (2 * (int64_t)num_cu + gy - 1) / gy;
        if (gx > N) gx = N;
        if (gx < 1) gx = 1;
        hipLaunchKernelGGL(score_rotation_grad_kernel, dim3((unsigned)gx, gy), dim3(kRotGradThreads), 0, stream, vol_src, R,
                           (long)r_batch_stride, W1, W2, b2, B, (long)N, du_ws, grad_R);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// d rotate_volume / d R (ahv_rotate_volume_rotation_grad_f32): the gather of score_rotation_grad_kernel with the upstream
// gradient READ instead of formed.  There dX = W1^T du comes out of MFMAs; here it is grad_out[n], the 32 KiB the op-level
// caller holds in HBM, and nothing else changes:
//   grad_R[n][a][b] = sum_p ( sum_c grad_out[n][c][p] * d out[n][c][p] / d i_a ) * (S_a / 2) * p_b
// with p = (x_w, y_h, z_d) the voxel centres, i_a = ((R_n p)_a + 1) S_a / 2 - 1/2, S = (W, H, D), and the conventions of
// ahv_trilinear.h (floor(i) is the cell, an outside corner contributes nothing, the coordinate is clamped before the
// conversion).  The forward and the volume adjoint are ahv_rotate.hip.
// (16, 8, 8, 8): the same team -- one workgroup of four waves per hypothesis, wave m = channels 4 m .. 4 m + 3, the source
// channel-last in LDS, staged once per workgroup when the volume is shared (vol_batch_stride = 0) and once per hypothesis
// otherwise.  A lane owns the voxels (d, y = lane >> 3, x = lane & 7), d = 0 .. 7: its 32 words of grad_out are 32 loads of
// which each is one 256-byte run per wave, all issued before the first corner is read.  Nine sums per hypothesis: lane
// sums over d = 0 .. 7 in that order, a xor butterfly inside the wave, (w0 + w1) + (w2 + w3) through LDS.  No atomics, one
// workgroup per hypothesis always: the nine numbers are the same bits whatever N, the grid or the cut into calls are.
// Any other shape: one workgroup per hypothesis too, threads stride over the voxels, everything from global memory, the
// same reduction.
// A hypothesis whose R holds a NaN / inf reports NaN (as autograd does; the clamp would hide it).  Non-finite voxels and
// upstream gradients are not looked for: they propagate through the in-range corners by IEEE arithmetic.
// ---------------------------------------------------------------------------------------------------
constexpr int kRvgThreads = 256;

__global__ __launch_bounds__(kRvgThreads) void rotate_volume_rotation_grad_16x8_kernel(
    const float* __restrict__ grad_out, const float* __restrict__ vol, long vol_batch_stride, const float* __restrict__ R,
    long N, float* __restrict__ grad_R)
{
    __shared__ __attribute__((aligned(16))) float lds_src[kSrcFloats];
    __shared__ float lds_red[4 * 12];
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* src_ch = lds_src + 4 * m;
    const bool shared = vol_batch_stride == 0;
    if (shared) {
        stage_src_volume(lds_src, vol, tid, kRvgThreads);
        __syncthreads();
    }
    for (long h = blockIdx.x; h < N; h += gridDim.x) {
        // the lane's words of grad_out[h]: channel 4 m + c, plane z at g[c][z]; requested ahead of the staging and of R
        const float* gp = grad_out + h * (16 * 512) + (4 * m) * 512 + lane;
        float g[4][8];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int z = 0; z < 8; ++z) g[c][z] = gp[c * 512 + z * 64];
        if (!shared) {
            stage_src_volume(lds_src, vol + h * vol_batch_stride, tid, kRvgThreads);
            __syncthreads();
        }
        float Rm[9];
        bool bad_r;
        load_rotation(Rm, bad_r, R + h * 9);
        float sum[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) sum[i] = 0.0f;
        const float x4 = (float)(lane & 7) - 3.5f, y4 = (float)(lane >> 3) - 3.5f;   // 4 * voxel centre = S_a / 2 * p_b
#pragma unroll
        for (int z = 0; z < 8; ++z)
            rot_grad_voxel(sum, g[0][z], g[1][z], g[2][z], g[3][z], src_ch, Rm, x4, y4, (float)z - 3.5f);
        reduce_store_nine(sum, lds_red, tid, bad_r, grad_R + h * 9);
    }
}

__global__ __launch_bounds__(kRvgThreads) void rotate_volume_rotation_grad_generic_kernel(
    const float* __restrict__ grad_out, const float* __restrict__ vol, long vol_batch_stride, const float* __restrict__ R,
    long N, int C, int D, int H, int W, float* __restrict__ grad_R)
{
    __shared__ float lds_red[4 * 12];
    const int tid = threadIdx.x;
    const long plane = (long)D * H * W;
    const float sx = 0.5f * (float)W, sy = 0.5f * (float)H, sz = 0.5f * (float)D;   // d i_a / d q_a
    for (long n = blockIdx.x; n < N; n += gridDim.x) {
        float Rm[9];
        bool bad_r;
        load_rotation(Rm, bad_r, R + n * 9);
        const float* src = vol + n * vol_batch_stride;
        const float* go = grad_out + n * C * plane;
        float sum[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) sum[i] = 0.0f;
        for (long v = tid; v < plane; v += kRvgThreads) {
            const TriVoxel p = tri_voxel(v, D, H, W, Rm);
            TriAxis<long> ax, ay, az;
            tri_axis(tri_index(p.gx, W), W, 1L, ax);
            tri_axis(tri_index(p.gy, H), H, (long)W, ay);
            tri_axis(tri_index(p.gz, D), D, (long)W * H, az);
            long off[8];
            bool in[8];
            float s[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                off[k] = tri_corner_off(k, ax, ay, az);
                in[k] = tri_corner_in(k, ax, ay, az);
                s[k] = 0.0f;
            }
            for (int c = 0; c < C; ++c) {   // s_corner = <grad_out[:, p], V[:, corner]>; an outside corner is not read
                const float gc = go[c * plane + v];
                const float* sc = src + c * plane;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (in[k]) s[k] = fmaf(gc, sc[off[k]], s[k]);
            }
            float tx = 0.0f, ty = 0.0f, tz = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) tri_corner_grad(k, s[k], ax, ay, az, tx, ty, tz);
            tri_outer_add(sum, tx * sx, ty * sy, tz * sz, p.x, p.y, p.z);
        }
        reduce_store_nine(sum, lds_red, tid, bad_r, grad_R + n * 9);
    }
}

hipError_t launch_rotate_volume_rotation_grad(const float* grad_out, const float* vol, int64_t vol_batch_stride, const float* R,
                                              int64_t N, int C, int D, int H, int W, float* grad_R, int num_cu,
                                              hipStream_t stream)
{
    if (N == 0) return hipSuccess;
    if (C == 16 && D == 8 && H == 8 && W == 8) {
        int64_t blocks = 3 * (int64_t)num_cu;   // 47.7 KiB of LDS per workgroup: three per CU are resident
        if (blocks > N) blocks = N;
        hipLaunchKernelGGL(rotate_volume_rotation_grad_16x8_kernel, dim3((unsigned)blocks), dim3(kRvgThreads), 0, stream,
                           grad_out, vol, (long)vol_batch_stride, R, (long)N, grad_R);
    } else {
        int64_t blocks = 8 * (int64_t)num_cu;
        if (blocks > N) blocks = N;
        hipLaunchKernelGGL(rotate_volume_rotation_grad_generic_kernel, dim3((unsigned)blocks), dim3(kRvgThreads), 0, stream,
                           grad_out, vol, (long)vol_batch_stride, R, (long)N, C, D, H, W, grad_R);
    }
    return hipGetLastError();
}

}  // namespace ahv
