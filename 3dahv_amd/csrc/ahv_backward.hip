// ahv_backward.hip -- backward of the fused scorer (what Estimator.infoNCE_loss,
// modules/model_co3d.py:41-61, needs from autograd): given dL/dscore[b][n], the gradients w.r.t. the source
// volume, the target feature and the head weights.  (W.r.t. the rotations: ahv_rotgrad.hip, which starts from this file's
// head pass, launch_score_backward_head_du.)
//
//   scores[b][n] = 1/64 sum_pos <normalize(W2 relu(W1 slabs(rot(V_b, R_n))) + b2)[:, pos], tg_b[:, pos]>
//
// Four launches, nothing of the 32 KiB-per-hypothesis rotated volumes or 96 KiB slab tensors ever reaches HBM:
//   1.  score_backward_head_kernel   recomputes the forward of each hypothesis (same code as the forward
//       kernel), back-propagates through the score, the normalisation, GEMM2 and the ReLU and leaves
//       du = dL/du (32 x 64 floats per hypothesis) in the caller's workspace; accumulates d feat_tgt, d W2, d b2.
//       (score_backward_head_saved_kernel instead takes u from the workspace, where the training forward left it.)
//   2a. score_backward_w1_kernel     re-gathers each quarter of the rotated volume, dW1 += du X^T in registers;
//       score_backward_w1_reduce_kernel sums the workgroups' partials.
//   2b. score_backward_volume_rmw_kernel forms dX = W1^T du and scatters it through the trilinear weights into
//       private fp32 LDS images of dV (plain read-modify-writes), flushed once per sample (ahv_bwd_volume.hip).
// Kernels 1, 1', 2a and the reduce are here; what the two head kernels share is the head rule of ahv_bwd.h.
// All contractions are fp32 MFMA 16x16x4 (one float per lane and operand, so any LDS layout can feed them).
// Accumulation across waves/workgroups uses float atomics: gradients are reproducible to rounding, not bitwise.
// Accumulation targets are zeroed by launch_zero_fill (ahv_ops.hip), never by hipMemsetAsync (not graph-safe here).
// The LDS-atomic dV kernel of rounds 2-5 that 2b replaced is described in HISTORY.md (code: commit 86a1f1c).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ahv_bwd.h"
#include "ahv_launch.h"

namespace ahv {

constexpr int kBwdThreads = 256;  // 4 waves, one per SIMD: 512 registers per wave

// ---------------------------------------------------------------------------------------------------
// Kernel 1: forward recompute + backward through score / normalise / GEMM2 / ReLU.
// ---------------------------------------------------------------------------------------------------
// ACCUM = false (the rotation gradient, ahv_score_rotation_grad_f32): the pass that only leaves du in the workspace -- nothing
// is summed across hypotheses, no float atomics, so du (and all that follows from it) is a function of the hypothesis alone,
// bit for bit; grad_scores may then be null (= all ones) and the three gradient pointers are not touched.
template <bool ACCUM>
__global__ __launch_bounds__(kBwdThreads, 1) void score_backward_head_kernel(
    const float* __restrict__ vol_src, const float* __restrict__ feat_tgt, const float* __restrict__ R,
    long r_batch_stride, const float* __restrict__ W1, const float* __restrict__ W2, const float* __restrict__ b2,
    int B, long N, const float* __restrict__ grad_scores, float* __restrict__ du_ws,
    float* __restrict__ grad_feat_tgt, float* __restrict__ grad_W2, float* __restrict__ grad_b2)
{
    __shared__ __attribute__((aligned(1024))) float lds_src[kSrcFloats];  // at LDS address 0: see ahv_score.hip
    __shared__ __attribute__((aligned(16))) float lds_w1[kW1TableFloats];
    __shared__ __attribute__((aligned(16))) float lds_q[4 * kQuarterFloats];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4, row = lane & 15;
    float* buf = lds_q + wave * kQuarterFloats;

    stage_w1_table(lds_w1, W1, tid, kBwdThreads);
    DualFrags f;
    load_dual_frags(f, W2, b2, lane);
    const GatherLane glane = gather_lane(lane);
    const GatherDst gdst = gather_dst_swizzled(lane);
    float a2t[2][4][2];
    load_a2t(a2t, W2, lane);
    HeadSums sums;
    head_sums_zero(sums);

    const long hstep = (long)gridDim.x * 4;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        __syncthreads();
        stage_src_volume(lds_src, vol_src + (long)b * (16 * 512), tid, kBwdThreads);
        __syncthreads();
        f32x4 tg[4][2], dtg[4][2];
        {
            const float* ft = feat_tgt + (long)b * (32 * 64);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tg[t][m2][r] = ft[(16 * m2 + 4 * kq + r) * 64 + 16 * t + n];
                        dtg[t][m2][r] = 0.0f;
                    }
        }
        const float* Rb = R + (long)b * r_batch_stride;
        for (long h = (long)wave * gridDim.x + xcd_residue(blockIdx.x, gridDim.x, gridDim.y); h < N; h += hstep) {
            float Rm[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Rm[i] = Rb[h * 9 + i];
            f32x4 acc[2][4];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            {   // forward recompute: the fused scorer's pipelined gather / GEMM1 (ahv_dual.h)
                GatherHyp gh;
                gather_hyp(gh, Rm, glane);
                HatState st;
                // quarters in the scorer's order 0, 3, 1, 2 (quarter 3 - Q is the point mirror of Q and reuses its set-up)
                hat_prologue<0>(st, lds_src, gh);
                hat_body(st, buf, gdst); wave_lds_fence();
                gemm1_quarter_pipe<0>(acc, lds_w1, buf, lane, [&] { hat_prologue_mirror(st, lds_src); }); wave_lds_fence();
                hat_body<true>(st, buf, gdst); wave_lds_fence();
                gemm1_quarter_pipe<3>(acc, lds_w1, buf, lane, [&] { hat_prologue<1>(st, lds_src, gh); }); wave_lds_fence();
                hat_body(st, buf, gdst); wave_lds_fence();
                gemm1_quarter_pipe<1>(acc, lds_w1, buf, lane, [&] { hat_prologue_mirror(st, lds_src); }); wave_lds_fence();
                hat_body<true>(st, buf, gdst); wave_lds_fence();
                gemm1_quarter_pipe<2>(acc, lds_w1, buf, lane, [] {}); wave_lds_fence();
            }
            f32x4 v[2][4];
            gemm2_dual(v, acc, f);

            // the head rule (ahv_bwd.h), tile by tile
            const float g = ((!ACCUM && !grad_scores) ? 1.0f : grad_scores[(long)b * N + h]) * (1.0f / 64.0f);
            f32x4 dv[2][4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                head_tile_backward<ACCUM, true>(v[0][t], v[1][t], tg[t][0], tg[t][1], g, dv[0][t], dv[1][t], dtg[t][0], dtg[t][1]);
            if (ACCUM) {
#pragma unroll
                for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sums.db2p[m2][r] += dv[m2][0][r] + dv[m2][1][r] + dv[m2][2][r] + dv[m2][3][r];
            }

            // du = dr where u > 0
            f32x4 du[2][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) head_tile_du(a2t, dv[0][t], dv[1][t], du[0][t], du[1][t]);
            float* dst = du_ws + ((long)b * N + h) * 2048;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[((t * 2 + m) * 64 + lane) * 4 + r] = acc[m][t][r] > 0.0f ? du[m][t][r] : 0.0f;

            if (!ACCUM) continue;
            // dW2 += dv relu(u)^T: the contraction runs over positions, so both operands go through the
            // wave's LDS image once (dv as A, relu(u) as B).
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) buf[dimg(16 * m2 + 4 * kq + r, 16 * t + n)] = dv[m2][t][r];
            wave_lds_fence();
            float av[2][16];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int s = 0; s < 16; ++s) av[mt][s] = buf[dimg(16 * mt + row, 4 * s + kq)];
            wave_lds_fence();
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) buf[dimg(16 * m + 4 * kq + r, 16 * t + n)] = fmaxf(acc[m][t][r], 0.0f);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float bv = buf[dimg(16 * nt + n, 4 * s + kq)];
                    sums.dW2[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][s], bv, sums.dW2[0][nt], 0, 0, 0);
                    sums.dW2[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1][s], bv, sums.dW2[1][nt], 0, 0, 0);
                }
            wave_lds_fence();
        }
        if (!ACCUM) continue;
        float* gft = grad_feat_tgt + (long)b * (32 * 64);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2) head_flush_tgt(gft, t, m2, dtg[t][m2], lane);
    }
    if (ACCUM) head_flush(sums, grad_W2, grad_b2, lane);
}

// ---------------------------------------------------------------------------------------------------
// Kernel 1', round 6: the same backward through score / normalise / GEMM2 / ReLU WITHOUT the forward recompute -- u comes from
// the workspace, where the training forward (ahv_score_hypotheses_train_f32) left it in the fragment layout
// [t][m][lane][r] (du_word).  That removes gather + GEMM1 (832 of 960 MFMAs and ~900 of 2 547 vector instructions per hypothesis) from
// the backward for 8 KB more HBM traffic per hypothesis in each direction.
// Everything here is independent per position tile t (16 of the 64 positions): a hypothesis is walked tile by tile with
// ~90 transient registers (the whole-hypothesis form of kernel 1 keeps 6 x 32 alive and ran one wave per SIMD at 506
// registers: 2.2 ms at B = 32 x 9 000 for 16 KB of traffic and 192 MFMAs per hypothesis).  The per-sample state that would
// need a dynamic register index moves to LDS: the target fragments (shared, read-only) and the wave's d feat_tgt accumulator
// (lane-linear 16-byte read-modify-writes).  512 threads: two waves per SIMD.
// ---------------------------------------------------------------------------------------------------
constexpr int kSavedThreads = 512;

__global__ __launch_bounds__(kSavedThreads, 2) void score_backward_head_saved_kernel(
    const float* __restrict__ feat_tgt, const float* __restrict__ W2, const float* __restrict__ b2,
    int B, long N, const float* __restrict__ grad_scores, float* __restrict__ du_ws,
    float* __restrict__ grad_feat_tgt, float* __restrict__ grad_W2, float* __restrict__ grad_b2)
{
    __shared__ __attribute__((aligned(16))) float lds_tg[4 * 2 * 64 * 4];        // target fragments [t][m2][lane][r]
    __shared__ __attribute__((aligned(16))) float lds_dtg[8 * 4 * 2 * 64 * 4];   // per wave: d feat_tgt, same layout
    __shared__ __attribute__((aligned(16))) float lds_tr[8 * 2 * 32 * 20];       // per wave: dv tile and relu(u) tile, [o][16 pos + 4 pad]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4, row = lane & 15;
    float* dtg = lds_dtg + wave * (4 * 2 * 64 * 4) + lane * 4;
    float* trd = lds_tr + wave * (2 * 32 * 20);   // dv tile
    float* tru = trd + 32 * 20;                   // relu(u) tile

    DualFrags f;
    load_dual_frags(f, W2, b2, lane);
    float a2t[2][4][2];
    load_a2t(a2t, W2, lane);
    HeadSums sums;
    head_sums_zero(sums);

    const long hstep = (long)gridDim.x * 8;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        __syncthreads();
        {   // target fragments of the sample: tg[t][m2][r] = ft[16 m2 + 4 kq + r][16 t + n], one (t, m2) per wave
            const float* ft = feat_tgt + (long)b * (32 * 64);
            const int t = wave >> 1, m2 = wave & 1;
            f32x4 x;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = ft[(16 * m2 + 4 * kq + r) * 64 + 16 * t + n];
            *reinterpret_cast<f32x4*>(lds_tg + ((t * 2 + m2) * 64 + lane) * 4) = x;
#pragma unroll
            for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(dtg + i * 256) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        long h = (long)wave * gridDim.x + xcd_residue(blockIdx.x, gridDim.x, gridDim.y);
        // u of (hypothesis, tile): two 16-byte loads per lane, requested a tile ahead (the last tile requests the next
        // hypothesis' first).  du overwrites u tile by tile, word for word (du_word): a tile's loads are consumed before its
        // stores are issued, and the other tiles live in other words.
        f32x4 un0 = f32x4{0.f, 0.f, 0.f, 0.f}, un1 = un0;
        if (h < N) {
            const float* up = du_ws + ((long)b * N + h) * 2048 + lane * 4;
            un0 = *reinterpret_cast<const f32x4*>(up);
            un1 = *reinterpret_cast<const f32x4*>(up + 256);
        }
        for (; h < N; h += hstep) {
            const float g = grad_scores[(long)b * N + h] * (1.0f / 64.0f);
            float* dst = du_ws + ((long)b * N + h) * 2048;
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                const f32x4 a0 = un0, a1 = un1;   // u[16 m + 4 kq + r][16 t + n], m = 0 / 1
                {
                    const bool last = t == 3;
                    const long hn = last ? (h + hstep < N ? h + hstep : h) : h;
                    const float* up = du_ws + ((long)b * N + hn) * 2048 + lane * 4 + (last ? 0 : t + 1) * 512;
                    if (!last || hn != h) {   // (never re-read this hypothesis' first tile: it already holds du)
                        un0 = *reinterpret_cast<const f32x4*>(up);
                        un1 = *reinterpret_cast<const f32x4*>(up + 256);
                    }
                }
                // v = W2 relu(u) + b2 for this tile
                f32x4 v0 = f.bias[0], v1 = f.bias[1];
                const f32x4 ru0 = relu4(a0), ru1 = relu4(a1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[0][r][0], ru0[r], v0, 0, 0, 0);
                    v1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[0][r][1], ru0[r], v1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[1][r][0], ru1[r], v0, 0, 0, 0);
                    v1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[1][r][1], ru1[r], v1, 0, 0, 0);
                }
                // the head rule (ahv_bwd.h) on this tile; d feat_tgt of the tile makes a round trip through the wave's LDS
                const f32x4 tg0 = *reinterpret_cast<const f32x4*>(lds_tg + ((t * 2 + 0) * 64 + lane) * 4);
                const f32x4 tg1 = *reinterpret_cast<const f32x4*>(lds_tg + ((t * 2 + 1) * 64 + lane) * 4);
                f32x4 dv0, dv1;
                {
                    f32x4 d0 = *reinterpret_cast<const f32x4*>(dtg + (t * 2 + 0) * 256);
                    f32x4 d1 = *reinterpret_cast<const f32x4*>(dtg + (t * 2 + 1) * 256);
                    head_tile_backward<true, false>(v0, v1, tg0, tg1, g, dv0, dv1, d0, d1);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sums.db2p[0][r] += dv0[r];
                        sums.db2p[1][r] += dv1[r];
                    }
                    *reinterpret_cast<f32x4*>(dtg + (t * 2 + 0) * 256) = d0;
                    *reinterpret_cast<f32x4*>(dtg + (t * 2 + 1) * 256) = d1;
                }
                // du = dr where u > 0
                f32x4 du0, du1;
                head_tile_du(a2t, dv0, dv1, du0, du1);
                f32x4 x0, x1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // (u != u: the forward's exact path saved NaN for a sample with a non-finite voxel or weight)
                    x0[r] = a0[r] > 0.0f ? du0[r] : (a0[r] == a0[r] ? 0.0f : a0[r]);
                    x1[r] = a1[r] > 0.0f ? du1[r] : (a1[r] == a1[r] ? 0.0f : a1[r]);
                }
                *reinterpret_cast<f32x4*>(dst + t * 512 + lane * 4) = x0;        // du over the tile's u, same words
                *reinterpret_cast<f32x4*>(dst + t * 512 + 256 + lane * 4) = x1;
                // dW2 += dv relu(u)^T over the tile's 16 positions: both operands through the wave's LDS tiles [o][pos]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    trd[(4 * kq + r) * 20 + n] = dv0[r];
                    trd[(16 + 4 * kq + r) * 20 + n] = dv1[r];
                    tru[(4 * kq + r) * 20 + n] = ru0[r];
                    tru[(16 + 4 * kq + r) * 20 + n] = ru1[r];
                }
                wave_lds_fence();
#pragma unroll
                for (int sp = 0; sp < 4; ++sp) {   // k-step: positions 4 sp + kq
                    const float av0 = trd[row * 20 + 4 * sp + kq], av1 = trd[(16 + row) * 20 + 4 * sp + kq];
                    const float bv0 = tru[n * 20 + 4 * sp + kq], bv1 = tru[(16 + n) * 20 + 4 * sp + kq];
                    sums.dW2[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0, bv0, sums.dW2[0][0], 0, 0, 0);
                    sums.dW2[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0, bv1, sums.dW2[0][1], 0, 0, 0);
                    sums.dW2[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1, bv0, sums.dW2[1][0], 0, 0, 0);
                    sums.dW2[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1, bv1, sums.dW2[1][1], 0, 0, 0);
                }
                wave_lds_fence();
            }
        }
        float* gft = grad_feat_tgt + (long)b * (32 * 64);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
                head_flush_tgt(gft, t, m2, *reinterpret_cast<const f32x4*>(dtg + (t * 2 + m2) * 256), lane);
    }
    head_flush(sums, grad_W2, grad_b2, lane);
}

// ---------------------------------------------------------------------------------------------------
// Kernels 2a / 2b.  Both walk the hypotheses again with du from the workspace.  They are separate launches
// because each carries persistent state next to a gather / scatter that wants ~100 registers more (2a: the dW1
// accumulators, 96 registers per wave since the output is split over the two waves of a SIMD; 2b: the W1^T fragments
// and the private dV images, which fill the LDS).
//   2a  score_backward_w1_kernel          re-gathers each quarter X of the rotated volume, dW1 += du X^T
//   2b  score_backward_volume_rmw_kernel  dX = W1^T du per half volume, dV += trilinear^T dX in private LDS images
//                                         of the sample's volume gradient, flushed once per sample
// ---------------------------------------------------------------------------------------------------

// LDS images of 2a, both LINEAR with a small pad so that every access is "per-lane base + compile-time constant"
// (one address register, immediate offsets) and the MFMA operand reads are at worst 2-way bank conflicts:
//   X[c][voxel = a0*64 + b*8 + e], kXwStride = 129 floats per channel plane (odd: the z slab's B operand, 16 lanes =
//   16 channels of one voxel, lands on 16 different banks);
//   du[o][pos], kDuStride = 68 floats per row (rows 4 apart sit 16 banks apart: the fragment-wise fill is conflict-free).
constexpr int kXwStride = 129;
constexpr int kXwFloats = 16 * kXwStride;
constexpr int kDuStride = 68;

// Kernel 2a runs TWO waves per SIMD.  The 192 accumulator registers of dW1 are what kept it at one wave per
// SIMD, where every LDS round trip and every VALU burst is exposed (the no-MFMA build of the one-wave kernel still
// took 0.75 of its 1.0 ms).  The OUTPUT is split instead: wave role r = wave / 4 owns the dW1 rows of m-tile r
// (96 accumulator registers) and needs only du rows 16 r .. 16 r + 15; waves w and w + 4 (same SIMD) walk the
// same hypotheses independently -- no barrier, each with its own X image -- so each hypothesis is gathered twice
// (the blend is ~1/6 of the per-hypothesis work) and in exchange the two waves of a SIMD drift apart and cover
// each other's latencies exactly as in the forward kernel.  (Sharing one gather per pair behind workgroup
// barriers was tried first: the barriers put both waves of a SIMD in the same phase and it ran 10 % SLOWER than
// one wave per SIMD.)
template <int DEPTH>
struct HatRing {
    f32x4 slot[DEPTH][4];
};

template <int S, int DEPTH>
__device__ __forceinline__ void hat_pass_request(HatRing<DEPTH>& rg, const HatVoxel& vx)
{
    const f32x4* row = reinterpret_cast<const f32x4*>(vx.base + hat_off(S & 7));
#pragma unroll
    for (int j = 0; j < 4; ++j) rg.slot[S % DEPTH][j] = row[j];
}

template <int S, int DEPTH>
struct HatPassSteps {  // the 8 corner steps of ONE voxel, source rows requested DEPTH steps ahead (cf. HatSteps, ahv_dual.h)
    static __device__ __forceinline__ void run(HatRing<DEPTH>& rg, const HatVoxel& vx, f32x2 (&o)[8])
    {
        __builtin_amdgcn_sched_barrier(0);
        const f32x2 wn = {vx.w[S], vx.w[S]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = rg.slot[S % DEPTH][j];
            const f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
            if (S == 0) {
                o[2 * j] = lo * wn;
                o[2 * j + 1] = hi * wn;
            } else {
                o[2 * j] = __builtin_elementwise_fma(lo, wn, o[2 * j]);
                o[2 * j + 1] = __builtin_elementwise_fma(hi, wn, o[2 * j + 1]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (S + DEPTH < 8) hat_pass_request<(S + DEPTH < 8 ? S + DEPTH : 0), DEPTH>(rg, vx);
        HatPassSteps<S + 1, DEPTH>::run(rg, vx, o);
    }
};
template <int DEPTH>
struct HatPassSteps<8, DEPTH> {
    static __device__ __forceinline__ void run(HatRing<DEPTH>&, const HatVoxel&, f32x2 (&)[8]) {}
};

template <int DEPTH, int ROW>
__device__ __forceinline__ void hat_one_pass(const HatVoxel& vx, float* dst)
{
    HatRing<DEPTH> rg;
    f32x2 o[8];
    hat_pass_request<0, DEPTH>(rg, vx);
    if (DEPTH > 1) hat_pass_request<(DEPTH > 1 ? 1 : 0), DEPTH>(rg, vx);
    if (DEPTH > 2) hat_pass_request<(DEPTH > 2 ? 2 : 0), DEPTH>(rg, vx);
    if (DEPTH > 3) hat_pass_request<(DEPTH > 3 ? 3 : 0), DEPTH>(rg, vx);
    static_assert(DEPTH <= 4, "prologue written out for up to four slots");
    HatPassSteps<0, DEPTH>::run(rg, vx, o);
#pragma unroll
    for (int c = 0; c < 16; ++c) dst[c * ROW] = o[c >> 1][c & 1];
}

// dW1 rows of ONE m-tile += du X^T on quarter Q, software-pipelined one chunk deep (operands of chunk k+1 requested
// before the MFMAs of chunk k; sched_barrier keeps hipcc from sinking the reads back to their uses).
//   chunks 0-7:  x and y slabs, k-step s = K / 2 (positions pl = 4 s + kq of tile Q), four k-tiles: 1 A value,
//                8 B values (4 k-tiles x {x, y}), 8 MFMAs
//   chunks 8-11: z slab, k-steps s = 4 (K-8) .. +3 (all 64 positions): 4 A values, 8 B values, 8 MFMAs
struct W1Chunk {
    float a[4];
    float b[8];
};
constexpr int kW1Chunks = 12;  // 8 half-steps of the x / y slabs + 4 groups of the z slab

template <int Q, int K>
__device__ __forceinline__ void w1_load(W1Chunk& ck, const float* da, const float* bx, const float* by, const float* bz)
{
    // da = dbuf + (16 m + row)*kDuStride + kq : A[row = o][k = pos];   bx = xbuf + i0*kXwStride + 8 kq + j;
    // by = xbuf + i0*kXwStride + kq + 8 j;   bz = xbuf + n*kXwStride + kq
    if (K < 8) {
        constexpr int s = K >> 1, k0 = 4 * (K & 1);  // k-step s (pa = s >> 1, pb = 4 (s & 1) + kq), k-tiles k0 .. k0 + 3
        ck.a[0] = da[16 * Q + 4 * s];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ck.b[2 * i] = bx[2 * (k0 + i) * kXwStride + (s >> 1) * 64 + 32 * (s & 1)];     // X[c = 2 kt + i0][(pa, pb, e = j)]
            ck.b[2 * i + 1] = by[2 * (k0 + i) * kXwStride + (s >> 1) * 64 + 4 * (s & 1)];  // X[c = 2 kt + i0][(pa, b = j, pb)]
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int s = 4 * (K - 8) + i;
            ck.a[i] = da[4 * s];
#pragma unroll
            for (int a0 = 0; a0 < 2; ++a0) ck.b[2 * i + a0] = bz[a0 * 64 + 4 * s];  // X[c = n][voxel = a0*64 + 4 s + kq]
        }
    }
}

template <int Q, int K>
__device__ __forceinline__ void w1_mfma(f32x4 (&ax)[8], f32x4 (&ay)[8], f32x4 (&az)[4][2], const W1Chunk& ck)
{
    if (K < 8) {
        constexpr int k0 = 4 * (K & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ax[k0 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ck.a[0], ck.b[2 * i], ax[k0 + i], 0, 0, 0);
            ay[k0 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ck.a[0], ck.b[2 * i + 1], ay[k0 + i], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int a0 = 0; a0 < 2; ++a0)
                az[Q][a0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ck.a[i], ck.b[2 * i + a0], az[Q][a0], 0, 0, 0);
    }
}

template <int Q, int K>
struct W1Pipe {
    static __device__ __forceinline__ void run(f32x4 (&ax)[8], f32x4 (&ay)[8], f32x4 (&az)[4][2], W1Chunk& cur,
                                               const float* da, const float* bx, const float* by, const float* bz)
    {
        W1Chunk nxt;
        __builtin_amdgcn_sched_barrier(0);
        if (K + 1 < kW1Chunks) w1_load<Q, K + 1>(nxt, da, bx, by, bz);
        w1_mfma<Q, K>(ax, ay, az, cur);
        if (K + 1 < kW1Chunks) {  // the next chunk's LDS reads between this chunk's MFMAs (ahv_dual.h, G1Pipe)
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (K + 1 < kW1Chunks) W1Pipe<Q, K + 1>::run(ax, ay, az, nxt, da, bx, by, bz);
    }
};
template <int Q>
struct W1Pipe<Q, kW1Chunks> {
    static __device__ __forceinline__ void run(f32x4 (&)[8], f32x4 (&)[8], f32x4 (&)[4][2], W1Chunk&, const float*,
                                               const float*, const float*, const float*) {}
};

template <int Q>
__device__ __forceinline__ void bwd_w1_quarter(f32x4 (&ax)[8], f32x4 (&ay)[8], f32x4 (&az)[4][2], const float* dbuf,
                                               const float* xbuf, int lane)
{
    const int n = lane & 15, kq = lane >> 4, row = lane & 15;
    const int i0 = n >> 3, j = n & 7;
    const float* da = dbuf + row * kDuStride + kq;  // the wave's 16 du rows
    const float* bx = xbuf + i0 * kXwStride + 8 * kq + j;
    const float* by = xbuf + i0 * kXwStride + kq + 8 * j;
    const float* bz = xbuf + n * kXwStride + kq;
    W1Chunk first;
    w1_load<Q, 0>(first, da, bx, by, bz);
    W1Pipe<Q, 0>::run(ax, ay, az, first, da, bx, by, bz);
}

// quarter Q of the rotated volume into this wave's X image, one pass (voxel) after the other
template <int Q>
__device__ __forceinline__ void w1_gather(float* xbuf, const float* srcT, const GatherHyp& gh, const GatherDst& dst)
{
    float* d0 = xbuf + dst.o0;
    __builtin_amdgcn_s_setprio(1);  // the gathering wave is latency-bound, its partner streams MFMAs (ahv_dual.h)
    HatVoxel vx;
    hat_voxel<Q>(vx, srcT, gh, 0);
    hat_one_pass<3, kXwStride>(vx, d0);
    hat_voxel<Q>(vx, srcT, gh, 1);
    hat_one_pass<3, kXwStride>(vx, d0 + 32);
    __builtin_amdgcn_s_setprio(0);
}

constexpr int kW1Threads = 512;
constexpr int kDuHalfFloats = 16 * kDuStride;

__global__ __launch_bounds__(kW1Threads, 2) void score_backward_w1_kernel(
    const float* __restrict__ vol_src, const float* __restrict__ R, long r_batch_stride, int B, long N,
    const float* __restrict__ du_ws, float* __restrict__ dw1_partials)
{
    __shared__ __attribute__((aligned(1024))) float lds_src[kSrcFloats];  // at LDS address 0: see ahv_score.hip
    // per wave: du rows 16 role .. 16 role + 15 (local rows 0 .. 15) and the X image; after the hypothesis loop the
    // same pool is the scratch of the in-workgroup reduction of the accumulators
    __shared__ __attribute__((aligned(16))) float lds_pool[8 * kDuHalfFloats + 8 * kXwFloats];
    static_assert(8 * kDuHalfFloats + 8 * kXwFloats >= 4 * 96 * 64, "reduction scratch");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slot = wave & 3, role = wave >> 2;  // waves w and w + 4 share a SIMD and a hypothesis list
    const int n = lane & 15, kq = lane >> 4;
    float* dbuf = lds_pool + wave * kDuHalfFloats;
    float* xbuf = lds_pool + 8 * kDuHalfFloats + wave * kXwFloats;
    const GatherLane glane = gather_lane(lane);
    const GatherDst gdst = gather_dst_linear(lane);
    f32x4 ax[8], ay[8], az[4][2];
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
        ax[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        ay[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int a0 = 0; a0 < 2; ++a0) az[q][a0] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long hstep = (long)gridDim.x * 4;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        __syncthreads();
        stage_src_volume(lds_src, vol_src + (long)b * (16 * 512), tid, kW1Threads);
        __syncthreads();
        const float* Rb = R + (long)b * r_batch_stride;
        long h = (long)slot * gridDim.x + xcd_residue(blockIdx.x, gridDim.x, gridDim.y);
        // this wave's half of du: the four fragments (t, m = role) of the hypothesis's 2048 floats (du_word) = rows 16 role ..
        f32x4 duh[4];
        if (h < N) {
            const f32x4* src = reinterpret_cast<const f32x4*>(du_ws + ((long)b * N + h) * 2048);
#pragma unroll
            for (int i = 0; i < 4; ++i) duh[i] = __builtin_nontemporal_load(src + (2 * i + role) * 64 + lane);
        }
        for (; h < N; h += hstep) {
            float Rm[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) Rm[i] = Rb[h * 9 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i)  // this hypothesis's du rows, requested one iteration ago: fragment (t = i, m = role)
#pragma unroll
                for (int r = 0; r < 4; ++r) dbuf[(4 * kq + r) * kDuStride + 16 * i + n] = duh[i][r];  // banks 16 kq + n + const
            {   // the next hypothesis's travel meanwhile
                const long hn = (h + hstep < N) ? h + hstep : h;
                const f32x4* src = reinterpret_cast<const f32x4*>(du_ws + ((long)b * N + hn) * 2048);
#pragma unroll
                for (int i = 0; i < 4; ++i) duh[i] = __builtin_nontemporal_load(src + (2 * i + role) * 64 + lane);
            }
            GatherHyp gh;
            gather_hyp(gh, Rm, glane);
            w1_gather<0>(xbuf, lds_src, gh, gdst); wave_lds_fence();
            bwd_w1_quarter<0>(ax, ay, az, dbuf, xbuf, lane); wave_lds_fence();
            w1_gather<1>(xbuf, lds_src, gh, gdst); wave_lds_fence();
            bwd_w1_quarter<1>(ax, ay, az, dbuf, xbuf, lane); wave_lds_fence();
            w1_gather<2>(xbuf, lds_src, gh, gdst); wave_lds_fence();
            bwd_w1_quarter<2>(ax, ay, az, dbuf, xbuf, lane); wave_lds_fence();
            w1_gather<3>(xbuf, lds_src, gh, gdst); wave_lds_fence();
            bwd_w1_quarter<3>(ax, ay, az, dbuf, xbuf, lane); wave_lds_fence();
        }
    }
    // Reduce the four waves of each role inside the workgroup (two rounds through LDS), then ONE wave per role
    // writes the workgroup's partial dW1 rows to the workspace; score_backward_w1_reduce_kernel sums the partials.
    // (Flushing every wave's 96 accumulator registers with float atomics put 12.6 M atomic adds on 12 288
    // addresses: 0.37 ms of a 1.07-ms kernel, independent of N.)
    float* scratch = lds_pool;
    auto put = [&](int w) {
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                scratch[((w * 96) + 4 * kt + r) * 64 + lane] = ax[kt][r];
                scratch[((w * 96) + 32 + 4 * kt + r) * 64 + lane] = ay[kt][r];
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int a0 = 0; a0 < 2; ++a0)
#pragma unroll
                for (int r = 0; r < 4; ++r) scratch[((w * 96) + 64 + 4 * (2 * q + a0) + r) * 64 + lane] = az[q][a0][r];
    };
    auto get = [&](int w) {
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ax[kt][r] += scratch[((w * 96) + 4 * kt + r) * 64 + lane];
                ay[kt][r] += scratch[((w * 96) + 32 + 4 * kt + r) * 64 + lane];
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int a0 = 0; a0 < 2; ++a0)
#pragma unroll
                for (int r = 0; r < 4; ++r) az[q][a0][r] += scratch[((w * 96) + 64 + 4 * (2 * q + a0) + r) * 64 + lane];
    };
    __syncthreads();
    if (slot >= 2) put((slot - 2) + 2 * role);
    __syncthreads();
    if (slot < 2) get(slot + 2 * role);
    __syncthreads();
    if (slot == 1) put(role);
    __syncthreads();
    if (slot == 0) {
        get(role);
        // dW1[o = 16 role + 4 kq + r][k]: x: k = 16 kt + n; y: 128 + 16 kt + n; z: 256 + n*8 + 2 q + a0
        float* part = dw1_partials + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (32 * 384);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* g = part + (16 * role + 4 * kq + r) * 384;
#pragma unroll
            for (int kt = 0; kt < 8; ++kt) {
                g[16 * kt + n] = ax[kt][r];
                g[128 + 16 * kt + n] = ay[kt][r];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int a0 = 0; a0 < 2; ++a0) g[256 + n * 8 + 2 * q + a0] = az[q][a0][r];
        }
    }
}

// grad_W1[i] += sum over the workgroups' partials; blockIdx.y slices the workgroups so that the 50 MB-scale read is
// spread over the chip (grad_W1 is zeroed beforehand; 16 float atomics per element).
__global__ __launch_bounds__(256) void score_backward_w1_reduce_kernel(const float* __restrict__ partials, int count,
                                                                       float* __restrict__ grad_W1)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int per = (count + gridDim.y - 1) / gridDim.y;
    const int lo = blockIdx.y * per, hi = min(lo + per, count);
    float acc = 0.0f;
    for (int w = lo; w < hi; ++w) acc += partials[(size_t)w * (32 * 384) + i];
    if (hi > lo) global_add(grad_W1 + i, acc);
}

// ---- host-side launcher -------------------------------------------------------------------------------
hipError_t launch_score_backward(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                 const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                 const float* grad_scores, float* du_ws, float* dw1_partials,
                                 float* grad_vol, float* grad_feat_tgt,
                                 float* grad_W1, float* grad_W2, float* grad_b2, int num_cu, hipStream_t stream, bool saved_u)
{
    hipError_t e;
    {   // accumulation targets: one zero-fill launch
        void* const ptrs[5] = {grad_vol, grad_feat_tgt, grad_W1, grad_W2, grad_b2};
        const size_t bytes[5] = {sizeof(float) * (size_t)B * 8192, sizeof(float) * (size_t)B * 2048, sizeof(float) * 32 * 384,
                                 sizeof(float) * 32 * 32, sizeof(float) * 32};
        if ((e = launch_zero_fill(ptrs, bytes, 5, stream)) != hipSuccess) return e;
    }
    if (B == 0 || N == 0) return hipSuccess;
    if (saved_u)   // du_ws holds u of every hypothesis (the training forward); the head kernel turns it into du in place
        hipLaunchKernelGGL(score_backward_head_saved_kernel, backward_grid(num_cu, B, N, kBwdHeadSavedPerWg), dim3(kSavedThreads),
                           0, stream, feat_tgt, W2, b2, B, (long)N, grad_scores, du_ws, grad_feat_tgt, grad_W2, grad_b2);
    else
        hipLaunchKernelGGL(score_backward_head_kernel<true>, backward_grid(num_cu, B, N, kBwdHeadPerWg), dim3(kBwdThreads), 0,
                           stream, vol_src, feat_tgt, R, (long)r_batch_stride, W1, W2, b2, B, (long)N, grad_scores, du_ws,
                           grad_feat_tgt, grad_W2, grad_b2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid_w1 = backward_grid(num_cu, B, N, kBwdW1PerWg);   // one partial per workgroup: see BackwardWs
    hipLaunchKernelGGL(score_backward_w1_kernel, grid_w1, dim3(kW1Threads), 0, stream, vol_src, R, (long)r_batch_stride,
                       B, (long)N, du_ws, dw1_partials);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(score_backward_w1_reduce_kernel, dim3(32 * 384 / 256, 16), dim3(256), 0, stream, dw1_partials,
                       (int)(grid_w1.x * grid_w1.y), grad_W1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_score_backward_volume(R, r_batch_stride, W1, B, N, du_ws, grad_vol, num_cu, stream);
}

hipError_t launch_score_backward_head_du(const float* vol_src, const float* feat_tgt, const float* R, int64_t r_batch_stride,
                                         const float* W1, const float* W2, const float* b2, int B, int64_t N,
                                         const float* grad_scores, float* du_ws, int num_cu, hipStream_t stream)
{
    hipLaunchKernelGGL(score_backward_head_kernel<false>, backward_grid(num_cu, B, N, kBwdHeadDuPerWg), dim3(kBwdThreads), 0,
                       stream, vol_src, feat_tgt, R, (long)r_batch_stride, W1, W2, b2, B, (long)N, grad_scores, du_ws,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr);
    return hipGetLastError();
}

}  // namespace ahv
