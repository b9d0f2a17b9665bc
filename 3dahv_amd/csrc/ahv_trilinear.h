// ahv_trilinear.h -- the trilinear rule of the op-level rotate_volume family (ahv_rotate.hip) and of score_rotation_grad_kernel
// and the rotation gradient of rotate_volume (both ahv_rotgrad.hip), stated once.
//
// Semantics = F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False) as called by utils.rotate_volume
// (utils.py:123-129).  Voxel (d, h, w) of a (D, H, W) volume:
//   p = ((2w+1)/W-1, (2h+1)/H-1, (2d+1)/D-1); g = R p; i = ((g+1)*S-1)/2 per axis, S = (W, H, D);
//   8 neighbours floor(i), floor(i)+1, each dropped when outside [0, S-1] (zeros padding per corner).  g[0] indexes W,
//   g[1] H, g[2] D.
// The conventions are the parity contract with the reference (and with grid_sampler_3d_backward for the gradients):
// floor(i) is the cell (at an integer coordinate the derivative is V[i + 1] - V[i]), a corner outside the volume gives
// neither value nor derivative, and the coordinate is clamped before the conversion to int.
// Shared here is the RULE on the unnormalised coordinate i.  How i is formed decides its bits and is not folded: explicit
// fmaf(..., 3.5f) chains for the (16,8,8,8) image in LDS (rot_grad_voxel), tri_index on a contracted R p in the generic
// kernels.  (The fused scorer's hat_axis, ahv_dual.h, and exact_axis, ahv_exact.h, are different expressions on purpose.)
#pragma once
#include "ahv_device.h"

namespace ahv {

template <typename Off>
struct TriAxis {
    float w0, w1;   // value weights of rows j, j + 1 (0 where the row is outside the volume)
    float d0, d1;   // their derivatives w.r.t. the sample coordinate (-1 / +1, 0 where outside): "in range" is d != 0
    Off o0, o1;     // clamped row index * stride (floats)
};

template <typename Off>
__device__ __forceinline__ void tri_axis(float i, int size, Off stride, TriAxis<Off>& a)
{
    i = fminf(fmaxf(i, -2.0f), (float)size + 1.0f);   // keeps the conversion defined for any R; all corners are outside there anyway
    const float fl = floorf(i), t = i - fl;
    const int i0 = (int)fl, i1 = i0 + 1;
    const bool in0 = i0 >= 0 && i0 < size, in1 = i1 >= 0 && i1 < size;
    a.w0 = in0 ? 1.0f - t : 0.0f;
    a.w1 = in1 ? t : 0.0f;
    a.d0 = in0 ? -1.0f : 0.0f;
    a.d1 = in1 ? 1.0f : 0.0f;
    a.o0 = (Off)min(max(i0, 0), size - 1) * stride;
    a.o1 = (Off)min(max(i1, 0), size - 1) * stride;
}

// the unnormalised coordinate of the generic kernels
__device__ __forceinline__ float tri_index(float g, int size) { return ((g + 1.0f) * (float)size - 1.0f) * 0.5f; }

// voxel v of a (D, H, W) volume: its centre p = (x, y, z) and g = R p
struct TriVoxel { float x, y, z, gx, gy, gz; };

__device__ __forceinline__ TriVoxel tri_voxel(long v, int D, int H, int W, const float* r)
{
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((long)W * H));
    TriVoxel p;
    p.x = (2.0f * w + 1.0f) / (float)W - 1.0f;
    p.y = (2.0f * h + 1.0f) / (float)H - 1.0f;
    p.z = (2.0f * d + 1.0f) / (float)D - 1.0f;
    p.gx = r[0] * p.x + r[1] * p.y + r[2] * p.z;
    p.gy = r[3] * p.x + r[4] * p.y + r[5] * p.z;
    p.gz = r[6] * p.x + r[7] * p.y + r[8] * p.z;
    return p;
}

// corner k = (dz, dy, dx) as bits (4, 2, 1): is it inside, and where
template <typename Off>
__device__ __forceinline__ bool tri_corner_in(int k, const TriAxis<Off>& ax, const TriAxis<Off>& ay, const TriAxis<Off>& az)
{
    return ((k & 1) ? ax.d1 : ax.d0) != 0.0f && ((k & 2) ? ay.d1 : ay.d0) != 0.0f && ((k & 4) ? az.d1 : az.d0) != 0.0f;
}

template <typename Off>
__device__ __forceinline__ Off tri_corner_off(int k, const TriAxis<Off>& ax, const TriAxis<Off>& ay, const TriAxis<Off>& az)
{
    return ((k & 1) ? ax.o1 : ax.o0) + ((k & 2) ? ay.o1 : ay.o0) + ((k & 4) ? az.o1 : az.o0);
}

// t_a += s * d w_k / d i_a for corner k, s = <upstream gradient, V[corner]> (0 for an outside corner)
template <typename Off>
__device__ __forceinline__ void tri_corner_grad(int k, float s, const TriAxis<Off>& ax, const TriAxis<Off>& ay,
                                                const TriAxis<Off>& az, float& tx, float& ty, float& tz)
{
    const float wx = (k & 1) ? ax.w1 : ax.w0, gx = (k & 1) ? ax.d1 : ax.d0;
    const float wy = (k & 2) ? ay.w1 : ay.w0, gy = (k & 2) ? ay.d1 : ay.d0;
    const float wz = (k & 4) ? az.w1 : az.w0, gz = (k & 4) ? az.d1 : az.d0;
    tx = fmaf(s, gx * (wy * wz), tx);
    ty = fmaf(s, gy * (wx * wz), ty);
    tz = fmaf(s, gz * (wx * wy), tz);
}

// sum[3 a + b] += t_a * p_b
__device__ __forceinline__ void tri_outer_add(float (&sum)[9], float tx, float ty, float tz, float x, float y, float z)
{
    sum[0] = fmaf(tx, x, sum[0]); sum[1] = fmaf(tx, y, sum[1]); sum[2] = fmaf(tx, z, sum[2]);
    sum[3] = fmaf(ty, x, sum[3]); sum[4] = fmaf(ty, y, sum[4]); sum[5] = fmaf(ty, z, sum[5]);
    sum[6] = fmaf(tz, x, sum[6]); sum[7] = fmaf(tz, y, sum[7]); sum[8] = fmaf(tz, z, sum[8]);
}

// One voxel of the rotation gradient on the (16,8,8,8) source image in LDS: g0..g3 = the upstream gradient of the wave's four
// channels at the voxel, src_ch = the image at the first of them, (x4, y4, z4) = 4 * voxel centre = S_a / 2 * p_b;
// i_a = 4 (R p)_a + 3.5 as the explicit FMA chains of the (16,8,8,8) kernels.
__device__ __forceinline__ void rot_grad_voxel(float (&sum)[9], float g0, float g1, float g2, float g3, const float* src_ch,
                                               const float* Rm, float x4, float y4, float z4)
{
    TriAxis<int> ax, ay, az;
    tri_axis(fmaf(Rm[0], x4, fmaf(Rm[1], y4, fmaf(Rm[2], z4, 3.5f))), 8, kSrcStride, ax);
    tri_axis(fmaf(Rm[3], x4, fmaf(Rm[4], y4, fmaf(Rm[5], z4, 3.5f))), 8, kSrcRowsY * kSrcStride, ay);
    tri_axis(fmaf(Rm[6], x4, fmaf(Rm[7], y4, fmaf(Rm[8], z4, 3.5f))), 8, kSrcPlaneRows * kSrcStride, az);
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src_ch + tri_corner_off(c, ax, ay, az));
        float s = fmaf(g3, v[3], fmaf(g2, v[2], fmaf(g1, v[1], g0 * v[0])));
        s = tri_corner_in(c, ax, ay, az) ? s : 0.0f;   // outside: the clamped row is not this corner's
        tri_corner_grad(c, s, ax, ay, az, tx, ty, tz);
    }
    tri_outer_add(sum, tx, ty, tz, x4, y4, z4);
}

// the nine entries of a rotation, and whether one is a NaN / inf: autograd's gradient is then NaN, the clamp would hide it
__device__ __forceinline__ void load_rotation(float (&Rm)[9], bool& bad_r, const float* __restrict__ r)
{
    bad_r = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rm[i] = r[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) bad_r = bad_r || non_finite(Rm[i]);
}

// the nine sums of a hypothesis from its four waves' lane sums: a xor butterfly inside the wave, (w0 + w1) + (w2 + w3) through
// lds_red (4 x 12 floats); NaN where ``bad``.  Every thread of the 256-thread workgroup calls it (two barriers).
__device__ __forceinline__ void reduce_store_nine(float (&sum)[9], float* lds_red, int tid, bool bad, float* dst)
{
    const int lane = tid & 63, m = tid >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        float x = sum[i];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
        sum[i] = x;
    }
    if (lane < 9) {
        float x = sum[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) x = lane == i ? sum[i] : x;
        lds_red[m * 12 + lane] = x;
    }
    __syncthreads();
    if (tid < 9) {
        const float x = (lds_red[tid] + lds_red[12 + tid]) + (lds_red[24 + tid] + lds_red[36 + tid]);
        dst[tid] = bad ? __builtin_nanf("") : x;
    }
    __syncthreads();   // lds_red, and the source image of a per-hypothesis volume, are free again
}

}  // namespace ahv
