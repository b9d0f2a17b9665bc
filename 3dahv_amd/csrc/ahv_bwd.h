// ahv_bwd.h -- what the backward kernels share, stated once: the workspace layout of u / du (du_word), the head rule of
// the two head kernels (ahv_backward.hip), and dX = W1^T du per half volume with its W1^T fragments (kernel 2b,
// ahv_bwd_volume.hip, and score_rotation_grad_kernel, ahv_rotgrad.hip).  The host side of the same family -- the grid rule
// and the workspace layout -- is ahv_launch.h (backward_grid, BackwardWs).
#pragma once
#include <hip/hip_runtime.h>

#include "ahv_device.h"
#define AHV_FP32_LOW_HALF  // these kernels leave registers free on their SIMDs: see low_half (ahv_dual.h)
#include "ahv_dual.h"

namespace ahv {

// u / du of one hypothesis in the workspace (2 048 floats): the MFMA accumulator layout of the scorer, tile by tile --
//   word(o, pos) = ((pos >> 4) * 2 + (o >> 4)) * 256 + (((o >> 2) & 3) * 16 + (pos & 15)) * 4 + (o & 3)
// i.e. [t][m][lane = 16 kq + n][r] for o = 16 m + 4 kq + r, pos = 16 t + n.  A wave writes and reads a (t, m) fragment with
// one 16-byte access per lane, the training forward's u and the head kernel's du share the words (du overwrites u tile
// by tile), and a lane that wants du[4 sp + kq][16 t + n] (kernel 2b) finds the 64 lanes' words in one 256-byte run.
__device__ __forceinline__ int du_word(int o, int pos)
{
    return ((pos >> 4) * 2 + (o >> 4)) * 256 + (((o >> 2) & 3) * 16 + (pos & 15)) * 4 + (o & 3);
}

// du image in LDS: du[o][pos] at o*64 + (pos ^ ((o & 7) << 2)).  The XOR keeps aligned groups of four
// positions together (float4 fills) and spreads rows over banks for the transposed reads (k = pos).
__device__ __forceinline__ int dimg(int o, int pos) { return o * 64 + (pos ^ ((o & 7) << 2)); }

__device__ __forceinline__ void global_add(float* p, float v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------
// The head rule: backward through score / normalise / GEMM2 for ONE position tile (16 of the 64 positions), and the
// flushes of what the head kernels sum.  Kernel 1 (whole hypothesis in registers) calls the tile rule for t = 0..3,
// kernel 1' (tile by tile, d feat_tgt in LDS) once per step of its walk: the schedules differ, the arithmetic is this.
// Fragment layout throughout: lane (n, kq), x[m2][r] = X[o2 = 16 m2 + 4 kq + r][pos = 16 t + n].
// ---------------------------------------------------------------------------------------------------

// A operands of dr = W2^T dv: A[row = o][k = o2]: [m2][r2][m] = W2[16 m2 + 4 kq + r2][16 m + row]
__device__ __forceinline__ void load_a2t(float (&a2t)[2][4][2], const float* __restrict__ W2, int lane)
{
    const int kq = lane >> 4, row = lane & 15;
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2)
#pragma unroll
            for (int m = 0; m < 2; ++m) a2t[m2][r2][m] = W2[(16 * m2 + 4 * kq + r2) * 32 + 16 * m + row];
}

struct HeadSums {
    f32x4 dW2[2][2];   // [mt][nt][r]: dW2[16 mt + 4 kq + r][16 nt + n]
    float db2p[2][4];  // [m2][r]: partial over this lane's columns of db2[16 m2 + 4 kq + r]
};

__device__ __forceinline__ void head_sums_zero(HeadSums& s)
{
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) s.dW2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) s.db2p[i][r] = 0.0f;
}

// score = 1/64 sum_pos <v / max(|v|, eps), tg>; F.normalize's clamp passes no gradient to the norm when it is below eps.
// In: the tile's v and tg (m2 = 0 / 1) and g = dL/dscore / 64.  Out: dv -- which is also the tile's increment of db2 -- and,
// if ACCUM, d feat_tgt of the tile += its increment.  The order of the lane's ss / dt sums is the caller's, and the only thing
// that is: both orders are pinned.  M2_OUTER (m2 = 0 then 1, r = 0..3 inside) is kernel 1's -- the rotation gradient that
// starts from its ACCUM = false pass is recorded bit for bit (tests/golden/rotate_kernels_recorded.npz, the srg_ family);
// r-outer with the two m2 paired is kernel 1''s, whose db2 is held to 5e-6 of the recomputing backward's
// (tests/test_gpu_backward.py, SAVED_RTOL) and with kernel 1's order misses it (5.8e-6 on the large_mixed set).
template <bool ACCUM, bool M2_OUTER>
__device__ __forceinline__ void head_tile_backward(const f32x4& v0, const f32x4& v1, const f32x4& tg0, const f32x4& tg1, float g,
                                                   f32x4& dv0, f32x4& dv1, f32x4& dtg0, f32x4& dtg1)
{
    float ss = 0.0f, dt = 0.0f;
    if (M2_OUTER) {
        const f32x4 v[2] = {v0, v1}, tg[2] = {tg0, tg1};
#pragma unroll
        for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ss += v[m2][r] * v[m2][r];
                dt += v[m2][r] * tg[m2][r];
            }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ss += v0[r] * v0[r] + v1[r] * v1[r];
            dt += v0[r] * tg0[r] + v1[r] * tg1[r];
        }
    }
    ss += __shfl_xor(ss, 16, 64); dt += __shfl_xor(dt, 16, 64);
    ss += __shfl_xor(ss, 32, 64); dt += __shfl_xor(dt, 32, 64);
    const float nrm = sqrtf(ss);
    const bool clamped = nrm < 1e-12f;
    const float inv = 1.0f / fmaxf(nrm, 1e-12f);
    const float c3 = clamped ? 0.0f : dt * inv * inv * inv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dv0[r] = g * (tg0[r] * inv - c3 * v0[r]);
        if (ACCUM) dtg0[r] += g * inv * v0[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dv1[r] = g * (tg1[r] * inv - c3 * v1[r]);
        if (ACCUM) dtg1[r] += g * inv * v1[r];
    }
}

// dr = W2^T dv for one tile (the accumulator registers of dv are the B operand); the caller keeps du = dr where u > 0
__device__ __forceinline__ void head_tile_du(const float (&a2t)[2][4][2], const f32x4& dv0, const f32x4& dv1, f32x4& du0, f32x4& du1)
{
    du0 = f32x4{0.f, 0.f, 0.f, 0.f};
    du1 = du0;
#pragma unroll
    for (int r2 = 0; r2 < 4; ++r2) {
        du0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[0][r2][0], dv0[r2], du0, 0, 0, 0);
        du1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[0][r2][1], dv0[r2], du1, 0, 0, 0);
    }
#pragma unroll
    for (int r2 = 0; r2 < 4; ++r2) {
        du0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[1][r2][0], dv1[r2], du0, 0, 0, 0);
        du1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[1][r2][1], dv1[r2], du1, 0, 0, 0);
    }
}

// a sample's d feat_tgt, fragment (t, m2), into the caller's gradient
__device__ __forceinline__ void head_flush_tgt(float* gft, int t, int m2, const f32x4& d, int lane)
{
    const int n = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) global_add(gft + (16 * m2 + 4 * kq + r) * 64 + 16 * t + n, d[r]);
}

// the wave's dW2 and db2 (summed over its lanes' columns first) into the caller's gradients
__device__ __forceinline__ void head_flush(const HeadSums& s, float* grad_W2, float* grad_b2, int lane)
{
    const int n = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) global_add(grad_W2 + (16 * mt + 4 * kq + r) * 32 + 16 * nt + n, s.dW2[mt][nt][r]);
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = s.db2p[m2][r];
#pragma unroll
            for (int sh = 8; sh >= 1; sh >>= 1) x += __shfl_xor(x, sh, 64);
            if (n == 0) global_add(grad_b2 + 16 * m2 + 4 * kq + r, x);
        }
}

// ---------------------------------------------------------------------------------------------------
// dX = W1^T du, half a volume at a time, by a team of four waves (wave m = channels 4 m .. 4 m + 3): kernel 2b scatters it,
// score_rotation_grad_kernel gathers against it.
// ---------------------------------------------------------------------------------------------------

// du of one hypothesis as MFMA B operands, straight from the workspace into registers: lane (n, kq) holds
// du[o = 4 sp + kq][pos = 16 t + n] for sp < 8, t < 4 -- 32 floats.  The x / y slabs of quarter Q use tile t = Q,
// the z slab all four tiles, so no LDS image of du is needed in this kernel.
struct DuRegs {
    float v[4][8];
};

__device__ __forceinline__ void load_du_regs(DuRegs& d, const float* __restrict__ du_hyp, int lane)
{
    // o = 4 sp + kq = 16 m + 4 kq' + r  =>  m = sp >> 2, kq' = sp & 3, r = kq: word (2 t + m) * 256 + (16 (sp & 3) + n) * 4 + kq
    const float* p = du_hyp + (lane & 15) * 4 + (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) d.v[t][sp] = p[(2 * t + (sp >> 2)) * 256 + (sp & 3) * 64];
}

// W1^T fragments of channels 4 m .. 4 m + 3 (A operands; lane (row, kq) holds W1[o = 4 sp + kq][k(row)]):
//   x / y: k = 32 m + 16 kt + row (+ 128)            rows = (channel 2 kt + (row >> 3), slab index row & 7)
//   z:     k = 256 + (4 m + (row & 3)) * 8 + depth   rows = (plane al = row >> 2, channel row & 3), depth = 2 H + (al & 1) + 4 (al >> 1)
struct W1tFrags {
    float wx[2][8], wy[2][8], wz[2][8];
};

__device__ __forceinline__ void load_w1t_frags(W1tFrags& f, const float* __restrict__ W1, int m, int lane)
{
    const int kq = lane >> 4, row = lane & 15;
#pragma unroll
    for (int sp = 0; sp < 8; ++sp) {
        const float* w = W1 + (4 * sp + kq) * 384;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            f.wx[kt][sp] = w[32 * m + 16 * kt + row];
            f.wy[kt][sp] = w[128 + 32 * m + 16 * kt + row];
        }
#pragma unroll
        for (int H = 0; H < 2; ++H) f.wz[H][sp] = w[256 + (4 * m + (row & 3)) * 8 + 2 * H + ((row >> 2) & 1) + 4 * (row >> 3)];
    }
}

// dX image of a wave: channel-last, word address = al * kXPlane + b * kXRow + e * 4 + channel.  A y row (8 voxels x 4 channels)
// is padded to 34 words and a plane to 274: the x / y slab updates walk b (or e) across the lanes of an MFMA tile, and with
// the unpadded strides (32 and 288 words, both multiples of the 32 banks) all 64 lanes of such an access met in 4 banks --
// SQ_LDS_BANK_CONFLICT 12.7 k of 20.5 k LDS cycles per hypothesis in the first version of this kernel.
constexpr int kXRow = 34;                 // (2 mod 8, and the plane 2 mod 16: the eight voxels of a scatter step -- 4 apart in b, e and
constexpr int kXPlane = 8 * kXRow + 2;    //  depth -- then read eight different 4-bank groups; rows are 8-byte aligned only, so 16 bytes
constexpr int kXbufWords = 4 * kXPlane;   //  travel as two halves)

// dX of this wave's four channels over half volume H (depth planes a = 2 H + (al & 1) + 4 (al >> 1), al = 0..3) into the
// channel-last image xbuf[al][b * 8 + e][4]: the z slab first (plain 16-byte stores: a lane's four accumulator rows ARE the
// four channels of one voxel), then the x and y slabs of the two quarters added on top.
template <int H>
__device__ __forceinline__ void rmw_dx_half(const W1tFrags& w1t, const DuRegs& du, float* xbuf, int lane)
{
    const float (&wx)[2][8] = w1t.wx, (&wy)[2][8] = w1t.wy, (&wz)[2][8] = w1t.wz;
    const int n = lane & 15, kq = lane >> 4;
    {
        float* zb = xbuf + kq * kXPlane + (n >> 3) * kXRow + (n & 7) * 4;  // voxel (al = kq, b = 2 t + (n >> 3), e = n & 7)
#pragma unroll
        for (int t = 0; t < 4; t += 2) {
            f32x4 d0 = f32x4{0.f, 0.f, 0.f, 0.f}, d1 = d0;
#pragma unroll
            for (int sp = 0; sp < 8; ++sp) {
                d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[H][sp], du.v[t][sp], d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[H][sp], du.v[t + 1][sp], d1, 0, 0, 0);
            }
            *reinterpret_cast<f32x2*>(zb + 2 * t * kXRow) = f32x2{d0[0], d0[1]};
            *reinterpret_cast<f32x2*>(zb + 2 * t * kXRow + 2) = f32x2{d0[2], d0[3]};
            *reinterpret_cast<f32x2*>(zb + 2 * (t + 1) * kXRow) = f32x2{d1[0], d1[1]};
            *reinterpret_cast<f32x2*>(zb + 2 * (t + 1) * kXRow + 2) = f32x2{d1[2], d1[3]};
        }
    }
    wave_lds_fence();
    // x and y slabs of the two quarters, added onto the z slab in LDS.  Block order x0, x1, y0, y1 (x / y slab of quarter
    // H + 2 j): the words a block adds onto are requested a block AHEAD -- 16 MFMAs hide the round trip; read just in front
    // of their MFMAs they cost the wave ~150 cycles per block on an LDS the scatters keep 70 % busy (in-kernel stamps:
    // 5.1 k cycles per half for 3.1 k cycles of MFMAs).  y j reads what x j wrote, so its request follows x j's stores.
    // x: channel 2 kt + (kq >> 1), voxel (al, b = n & 7, e = 4 (kq & 1) + r);  y: voxel (al, b = 4 (kq & 1) + r, e = n & 7)
    float* const rbx = xbuf + (kq >> 1) + (n >> 3) * kXPlane + (n & 7) * kXRow + 16 * (kq & 1);
    float* const rby = xbuf + (kq >> 1) + (n >> 3) * kXPlane + 4 * (kq & 1) * kXRow + (n & 7) * 4;
    auto rd = [&](float (&o0)[4], float (&o1)[4], const float* rb, int rs) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0[r] = rb[rs * r];
            o1[r] = rb[rs * r + 2];
        }
    };
    auto mm = [&](f32x4& d0, f32x4& d1, const float (&w)[2][8], int t) {
        d0 = f32x4{0.f, 0.f, 0.f, 0.f};
        d1 = d0;
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0][sp], du.v[t][sp], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1][sp], du.v[t][sp], d1, 0, 0, 0);
        }
    };
    auto wr = [&](float* rb, int rs, const float (&o0)[4], const float (&o1)[4], const f32x4& d0, const f32x4& d1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rb[rs * r] = o0[r] + d0[r];
            rb[rs * r + 2] = o1[r] + d1[r];
        }
        wave_lds_fence();   // (compiler-level: later reads of these words, by other lanes, stay behind the stores)
    };
    float ax0[4], ax1[4], bx0[4], bx1[4], ay0[4], ay1[4], by0[4], by1[4];
    f32x4 d0, d1;
    rd(ax0, ax1, rbx, 4);                          // x0
    rd(bx0, bx1, rbx + 2 * kXPlane, 4);            // x1
    mm(d0, d1, wx, H);
    wr(rbx, 4, ax0, ax1, d0, d1);
    rd(ay0, ay1, rby, kXRow);                      // y0 (behind x0's stores)
    mm(d0, d1, wx, H + 2);
    wr(rbx + 2 * kXPlane, 4, bx0, bx1, d0, d1);
    rd(by0, by1, rby + 2 * kXPlane, kXRow);        // y1 (behind x1's stores)
    mm(d0, d1, wy, H);
    wr(rby, kXRow, ay0, ay1, d0, d1);
    mm(d0, d1, wy, H + 2);
    wr(rby + 2 * kXPlane, kXRow, by0, by1, d0, d1);
}

}  // namespace ahv
