// ahv_enc_linear.h -- the GEMM kernels of the encoder, included by ahv_encoder.hip (one translation unit: no launcher
// prototypes, the probe globals stay file-static):
//
//   linear_staged_kernel  P[ks][M][N] = X[M][K-slice ks] . W[N][K-slice]^T   fp32 MFMA 16x16x4, split-K, up to 4
//                         problems per launch, K walked in stages through LDS; optional bias + GEGLU epilogue; the 3 x 3
//                         convolution with one tap per K slice
//   linear_kernel         the register-resident form of the same for the taps of the 3-D convolutions
//   linear_tile_kernel    128 x 128 tiles (M >= 1024: the FF projections), 64 x 64 tiles (M >= 2048: the 256-wide projections;
//                         the 3 x 3 convolutions as an implicit GEMM)
//
// fp32 throughout (the reference runs set_float32_matmul_precision("highest")).  Which of them a launch takes: ahv_enc_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ahv_enc_probe.h"

namespace ahv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// Output stores of the big launches (A/B on one box with tools/kbench_enc): the tile linear stores non-temporally, which
// leaves less dirty data in the L2s for the write-back at the end of a kernel, which sits between every two launches of
// this forward.  The row kernels (attention + output projection, LayerNorm / concat) store plainly: non-temporal stores
// there measured 1 910 / 1 909 against 1 901 / 1 905 us per forward at B = 32, 317 against 309 us at B = 1 (HISTORY.md).

constexpr int kMaxProb = 4;

struct LinProb {
    const float* X;     // [M][ldx]  (GEGLU mode: the [M][2H] slab of the previous linear)
    const float* W;     // [N][ldw]
    float* P;           // [KS][M][N]
    const float* bias;  // GEGLU: bias of this projection [2H]; plain, one K slice: bias [N] or null
    int N;
    int tile0;          // first n-tile of this problem in blockIdx.x
};

struct LinArgs {
    LinProb p[kMaxProb];
    int nprob, M, Kc;
    long ldx, ldw;
    int geglu_h;  // H > 0: GEGLU epilogue, W has 2H rows (value rows, then gate rows), output [M][H]
#ifdef AHV_ENC_PROBE
    unsigned long long* stamps;
#endif
};

// GELU(g) = g Phi(g), exact form (nn.GELU() default = 0.5 g (1 + erf(g / sqrt 2)), attention.py:81-88), for a PAIR of values
// on the packed fp32 pipe.  A 128 x 128 GEGLU tile ends in 64 of them per lane, and fp32 MFMAs do not overlap VALU work on
// gfx950: libdevice's erff (a branch between two polynomials, 35 vector instructions per value) cost the FF-in launch as
// much as 300 MFMAs per wave and tile, both ranges of a < 1-ulp erf on v_pk_fma_f32 (round 6, first form) 18 per value.
// This form needs 8:  GELU(g) = max(g, 0) - |g| Phi(-|g|)  with  Phi(-t) = exp2(p(t)),  p(t) = -1 + c1 t + ... + c8 t^8
// -- log2 of the normal tail is smooth on t >= 0, so ONE polynomial serves every t, c8 < 0 and p falls monotonically
// beyond the fitted [0, 6], so large |g| need no clamp (exp2 -> 0), and nothing cancels: for g > 0 the tail is subtracted
// from g, for g < 0 it IS the result (0.5 g (1 + erf) loses digits there).  tools/fit_gelu.py regenerates the
// coefficients and the error with fp32 rounding after every operation: |gelu_pk - fp64| <= 2.6e-7 on [-300, 300], where
// the expression torch evaluates in fp32 is off by up to 4.5e-7; relative to max(|GELU|, 1e-3) 1.7e-5 against 8.3e-5.
// (g = +inf gives NaN here -- inf * 0 -- and inf there; LayerNorm turns either into NaN one launch later.)
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define AHV_PK(c) (f32x2{c, c})
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ f32x2 gelu_pk(f32x2 g)
{
    const f32x2 t = __builtin_elementwise_abs(g);
    f32x2 r = pk_fma(AHV_PK(-2.357509857e-06f), t, AHV_PK(3.389861013e-05f));
    r = pk_fma(r, t, AHV_PK(-1.614213979e-04f));
    r = pk_fma(r, t, AHV_PK(-1.932584128e-04f));
    r = pk_fma(r, t, AHV_PK(7.131781429e-03f));
    r = pk_fma(r, t, AHV_PK(-5.253926665e-02f));
    r = pk_fma(r, t, AHV_PK(-4.591956735e-01f));
    r = pk_fma(r, t, AHV_PK(-1.151106358e+00f));
    r = pk_fma(r, t, AHV_PK(-1.0f));
    const f32x2 tail = {__builtin_amdgcn_exp2f(r[0]), __builtin_amdgcn_exp2f(r[1])};   // Phi(-|g|)
    const f32x2 pos = {fmaxf(g[0], 0.0f), fmaxf(g[1], 0.0f)};
    return pk_fma(-t, tail, pos);
}

// (v0, v1) * GELU(g0, g1)
__device__ __forceinline__ f32x2 geglu_pk(f32x2 v, f32x2 g) { return v * gelu_pk(g); }

// -------------------------------------------------------------------------------------------------
// Skinny linear, register-resident: the 3 x 3 x 3 convolutions over the 8^3 voxels of a channel-last volume as an implicit
// GEMM.  grid = (sum of n-tiles, KS, M / 64); 512 threads.  The workgroup owns 64 rows x 16 columns and the K range
// [ks*Kc, (ks+1)*Kc); its 8 waves split that range (KW columns each, every W row segment is streamed exactly once).  The K
// axis is (tap, channel) with C = KW channels, so a wave has one tap: the row a lane reads is its own voxel shifted by the
// tap, or zero outside the volume (zero padding).  Taps >= 27 are K padding: their weights are zero and nothing is loaded.
// Both MFMA operands go straight from memory to registers: with the k ordering "MFMA k-step s, lane group kq <-> column
// k0 + 4*kq + s" a lane needs exactly one aligned float4 of its X row and one of its W row per 16-wide step, and nobody
// else needs them.  ALL loads of a wave are issued before its first MFMA (sched_barrier keeps hipcc from sinking them to
// their uses), so the memory latency is paid once.  The 8 partial tiles meet in LDS.
// -------------------------------------------------------------------------------------------------
template <int KW>
__global__ __launch_bounds__(512) void linear_kernel(const LinArgs a)
{
    __shared__ __attribute__((aligned(16))) float red[8 * 64 * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    AHV_ENC_STAMP(0);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxProb; ++i)
        if (i < a.nprob && (int)blockIdx.x >= a.p[i].tile0) pi = i;
    const LinProb pr = a.p[pi];
    const int tile = (int)blockIdx.x - pr.tile0;
    const int n0 = tile * 16;
    const int ks = blockIdx.y;
    const int m0 = blockIdx.z * 64;
    const int kbase = ks * a.Kc + wave * KW;
    const int r16 = lane & 15, kq = lane >> 4;
    constexpr int STEPS = KW / 16;

    f32x4 w[STEPS], x[STEPS][4];
    const float* xsrc[4];
    bool xok[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int p = rt * 16 + r16;  // row of this lane inside the 64-row tile
        const int tap = kbase / KW;
        const int v = (m0 & 511) + p;  // voxel inside the sample
        const int nd = (v >> 6) + tap / 9 - 1, nh = ((v >> 3) & 7) + (tap / 3) % 3 - 1, nw = (v & 7) + tap % 3 - 1;
        xok[rt] = tap < 27 && (unsigned)nd < 8u && (unsigned)nh < 8u && (unsigned)nw < 8u;
        xsrc[rt] = pr.X + (long)((m0 - (m0 & 511)) + (xok[rt] ? nd * 64 + nh * 8 + nw : v)) * KW + 4 * kq;
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
        w[st] = *reinterpret_cast<const f32x4*>(pr.W + (long)(n0 + r16) * a.ldw + kbase + 16 * st + 4 * kq);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            x[st][rt] = *reinterpret_cast<const f32x4*>(xsrc[rt] + 16 * st);
            if (!xok[rt]) x[st][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < STEPS; ++st)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[st][rt][s4], w[st][s4], acc[rt], 0, 0, 0);
    AHV_ENC_STAMP(4);
    // cross-wave reduction through LDS, then one coalesced store
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            red[(wave * 64 + rt * 16 + 4 * kq + r) * 16 + r16] = acc[rt][r];
    __syncthreads();
    AHV_ENC_STAMP(5);
    float* out = pr.P + ((long)ks * a.M + m0) * pr.N + n0;
    for (int i = tid; i < 64 * 16; i += 512) {
        const int r = i / 16, c = i - r * 16;
        float v = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 8; ++wv) v += red[i + wv * 64 * 16];
        out[(long)r * pr.N + c] = v;
    }
    AHV_ENC_STAMP(6);
}

// -------------------------------------------------------------------------------------------------
// The same linear, K-PIPELINED through LDS (MODE 0 / 1; grid, LinArgs and 512 threads as linear_kernel).
// linear_kernel requests its whole operand set at once and as MFMA fragments: the four lanes of a quad then sit
// in four different 128-byte lines and the texture path delivers ~16 B/clk (tools/launch_floor.cpp: 128 KB re-read
// per workgroup 3.3 us as fragments, 1.15 us row-contiguous), so a workgroup of the FF-in projection spends ~5 us
// receiving 192 KB before its last wave can start its MFMAs, and ends with an 8-way reduction through LDS.
// Here the workgroup walks K in stages of 64 columns: X[64][64] and W[16 NT][64] are fetched row-contiguously
// (16 lanes = one 256-byte row segment), parked in a double-buffered LDS stage (row stride 68 floats: a fragment
// read of 16 rows x one float4 covers all 64 banks once) while the MFMAs of the previous stage run, and wave w
// owns output rows 16 w .. 16 w + 15 over ALL of the workgroup's columns and ALL of K -- no cross-wave reduction,
// and the value and gate tiles of the GEGLU projection meet in one lane's registers.
// -------------------------------------------------------------------------------------------------
constexpr int kStageK = 64;    // K columns per stage
constexpr int kStageLd = 68;   // floats per staged row

template <int NT, int KC, bool GEGLU_OUT, int MODE = 0>
__global__ __launch_bounds__(512) void linear_staged_kernel(const LinArgs a)
{
    static_assert(MODE == 0 || MODE == 1, "MODE 2 (3-D taps) stays with linear_kernel");
    static_assert(GEGLU_OUT ? NT == 2 : NT == 1, "one n-tile per workgroup, or the value and the gate tile of the GEGLU projection");
    constexpr int NS = KC / kStageK;  // stages
    constexpr int DEPTH = 2 < NS ? 2 : NS;  // stages requested ahead of their use (3, 4, 8 measured: 319.7 / 323.9 / 323.9 us
                                            // per forward against 318.5 at 2, round 3)
    // two stage buffers (26 KB each at NT = 2): 2 workgroups per CU once M > 64.  (Three buffers with the next stage's
    // fragments read between this stage's MFMAs: equal at B = 1 -- 309.2 against 309.4 us per forward --, 4-10 % slower at
    // B = 2..8, measured again in round 5 on the interleaved issue order below.)
    __shared__ __attribute__((aligned(16))) float sx[2][64 * kStageLd];
    __shared__ __attribute__((aligned(16))) float sw[2][16 * NT * kStageLd];
    __shared__ __attribute__((aligned(16))) float comb[4 * 64 * 4];  // the second wave of each pair hands its tile over
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Two waves per SIMD (a lone wave issues an fp32 MFMA only every ~40 cycles): wave = (row tile rt, half h).
    // NT = 2 (GEGLU): h = n-tile (0 value, 1 gate).  NT = 1: h = half of every stage's K (k-steps 2h, 2h + 1).
    const int rt = wave & 3, half = wave >> 2;
    AHV_ENC_STAMP(0);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxProb; ++i)
        if (i < a.nprob && (int)blockIdx.x >= a.p[i].tile0) pi = i;
    const LinProb pr = a.p[pi];
    const int tile = (int)blockIdx.x - pr.tile0;
    const int n0 = GEGLU_OUT ? tile * 16 : tile * 16 * NT;
    const int nstep = GEGLU_OUT ? a.geglu_h : 16;  // distance between the workgroup's n-tiles
    const int ks = blockIdx.y;
    const int m0 = blockIdx.z * 64;
    const int r16 = lane & 15, kq = lane >> 4;

    // staging map: thread -> (row tid / 16 (+32), float4 column tid % 16); W: 16 NT rows, the first 256 NT threads
    const int srow = tid >> 4, sc4 = (tid & 15) * 4;
    const float* xg[2];
    bool xok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = srow + 32 * j;  // row inside the 64-row tile
        if (MODE == 0) {
            xg[j] = pr.X + (long)(m0 + p) * a.ldx + (long)ks * KC + sc4;
            xok[j] = true;
        } else {  // 3x3 convolution over 8x8 tokens: this K slice is tap ks, all 256 channels
            const int ny = (p >> 3) + ks / 3 - 1, nx = (p & 7) + ks % 3 - 1;
            xok[j] = (unsigned)ny < 8u && (unsigned)nx < 8u;
            xg[j] = pr.X + (long)(m0 + (xok[j] ? ny * 8 + nx : p)) * 256 + sc4;
        }
    }
    const bool wload = srow < 16 * NT;
    const int wrow = wload ? srow : 0;
    const float* wg = pr.W + (long)(n0 + (wrow >> 4) * nstep + (wrow & 15)) * a.ldw + (long)ks * KC + sc4;

    f32x4 gx[NS][2], gw[NS];
    auto request = [&](int st) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            gx[st][j] = xok[j] ? *reinterpret_cast<const f32x4*>(xg[j] + kStageK * st) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (wload) gw[st] = *reinterpret_cast<const f32x4*>(wg + kStageK * st);
    };
    auto park = [&](int st, int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(&sx[buf][(srow + 32 * j) * kStageLd + sc4]) = gx[st][j];
        if (wload) *reinterpret_cast<f32x4*>(&sw[buf][srow * kStageLd + sc4]) = gw[st];
    };
#pragma unroll
    for (int st = 0; st < DEPTH; ++st) request(st);
    float gbias_v = 0.0f, gbias_g = 0.0f;  // GEGLU epilogue: this lane's column
    if (GEGLU_OUT) {
        gbias_v = pr.bias[n0 + r16];
        gbias_g = pr.bias[a.geglu_h + n0 + r16];
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int KSTEPS = NT == 2 ? 4 : 2;        // k-steps of 16 per stage and wave
    const int k40 = NT == 2 ? 0 : 2 * half;        // first of them
    const int wtile = NT == 2 ? half : 0;          // n-tile of this wave
    park(0, 0);
    __syncthreads();
    AHV_ENC_STAMP(3);
#pragma unroll
    for (int st = 0; st < NS; ++st) {
        const int cur = st & 1;
        // issue order: this stage's fragment reads first, then its (dependent, ~40 cycles apart) MFMAs with the requests of
        // stage st + DEPTH and the LDS stores of stage st + 1 in the gaps between them (hard fences: sched_group_barrier
        // does not move instructions the MFMAs' own operands depend on)
        __builtin_amdgcn_sched_barrier(0);
        f32x4 fx[KSTEPS], fw[KSTEPS];
#pragma unroll
        for (int k = 0; k < KSTEPS; ++k) {
            fx[k] = *reinterpret_cast<const f32x4*>(&sx[cur][(16 * rt + r16) * kStageLd + 16 * (k40 + k) + 4 * kq]);
            fw[k] = *reinterpret_cast<const f32x4*>(&sw[cur][(16 * wtile + r16) * kStageLd + 16 * (k40 + k) + 4 * kq]);
        }
        __builtin_amdgcn_sched_barrier(0);
        constexpr int NM = 4 * KSTEPS;  // MFMAs of this stage
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fx[q >> 2][q & 3], fw[q >> 2][q & 3], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            const int slot = q;  // one memory instruction behind each of the first six MFMAs
            if (st + DEPTH < NS) {
                const int sr = st + DEPTH;
                if (slot == 0) gx[sr][0] = xok[0] ? *reinterpret_cast<const f32x4*>(xg[0] + kStageK * sr) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (slot == 1) gx[sr][1] = xok[1] ? *reinterpret_cast<const f32x4*>(xg[1] + kStageK * sr) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (slot == 2 && wload) gw[sr] = *reinterpret_cast<const f32x4*>(wg + kStageK * sr);
            }
            if (st + 1 < NS) {
                const int sp = st + 1, buf = cur ^ 1;
                if (slot == 3) *reinterpret_cast<f32x4*>(&sx[buf][srow * kStageLd + sc4]) = gx[sp][0];
                if (slot == 4) *reinterpret_cast<f32x4*>(&sx[buf][(srow + 32) * kStageLd + sc4]) = gx[sp][1];
                if (slot == 5 && wload) *reinterpret_cast<f32x4*>(&sw[buf][srow * kStageLd + sc4]) = gw[sp];
            }
            if (slot < 6) __builtin_amdgcn_sched_barrier(0);
        }
        if (st + 1 < NS) __syncthreads();
    }
    AHV_ENC_STAMP(4);
    // D layout: acc[r] = C[m0 + 16 rt + 4 kq + r][column r16 of this wave's n-tile]; waves 4..7 hand over
    if (half == 1) *reinterpret_cast<f32x4*>(&comb[(rt * 64 + lane) * 4]) = acc;
    __syncthreads();
    if (half == 0) {
        const f32x4 other = *reinterpret_cast<const f32x4*>(&comb[(rt * 64 + lane) * 4]);
        if (GEGLU_OUT) {
            float* out = pr.P + (long)(m0 + 16 * rt + 4 * kq) * a.geglu_h + n0 + r16;
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const f32x2 y = geglu_pk(f32x2{acc[r] + gbias_v, acc[r + 1] + gbias_v}, f32x2{other[r] + gbias_g, other[r + 1] + gbias_g});
                out[(long)r * a.geglu_h] = y[0];
                out[(long)(r + 1) * a.geglu_h] = y[1];
            }
        } else {
            float* out = pr.P + ((long)ks * a.M + m0 + 16 * rt + 4 * kq) * pr.N + n0 + r16;
            const float bias = pr.bias ? pr.bias[n0 + r16] : 0.0f;  // a 1x1 conv's bias (single K slice only: host)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long)r * pr.N] = acc[r] + other[r] + bias;
        }
    }
    AHV_ENC_STAMP(6);
}

// -------------------------------------------------------------------------------------------------
// Tiled linear for MANY rows (M >= 1024, i.e. B >= 16): C[M][N] = X[M][K] . W[N][K]^T, fp32 MFMA 16x16x4.
// The skinny kernels above give a workgroup 64 rows x 16 or 32 columns and re-read its X rows once per column tile:
// right for 64..512 rows (weights are the traffic), 44 % of the matrix peak at 2048 rows (measured on the
// register-resident form, which also pays an 8-way LDS reduction per output tile).  Here a
// workgroup (256 threads, 2 x 2 waves) owns a 128 x 128 output tile and walks K in steps of 16 through three
// LDS stages; a wave owns 64 x 64 (16 accumulator tiles).  Both operands are K-contiguous, so
// a tile row in LDS is one 64-byte line [16 k] and, with the k ordering "MFMA k-step s, lane group kq <-> k = 4 kq
// + s", an operand fragment is one lane-linear (conflict-free) ds_read_b128 serving four MFMA k-steps.
// GEGLU (the FF-in projection, attention.py:81-88): the 128 tile columns are, per wave column wc, 32 VALUE columns
// and their 32 GATE columns, so value and gate of one output element sit in the same lane and the epilogue writes
// (v + b_v) * gelu(g + b_g) straight into the [M][H] buffer.
// -------------------------------------------------------------------------------------------------
struct TileArgs {
    LinProb p[kMaxProb];  // tile0 = first column tile of the problem in blockIdx.x
    int nprob, M, K;      // K = K range of ONE split (blockIdx.z = ks)
    long ldx, ldw;
    int geglu_h;
    const float* zero;    // CONV: 64 bytes of zeros (what a tap outside the 8 x 8 image reads)
#ifdef AHV_ENC_PROBE
    unsigned long long* stamps;
#endif
};

// K pipeline (round 5): four LDS stages filled by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write --
// the stage image is lane-linear, thread t owns bytes [16 t, 16 t + 16) of each 4 KiB piece, which is exactly what one
// such instruction per wave writes), two fragment sets.  In k-step kt a wave requests tile kt + 3, reads the fragments of
// tile kt + 1 from LDS, issues the MFMAs of tile kt (whose fragments it read a k-step ago), waits until its own pieces of
// tile kt + 2 have landed (vmcnt: tile kt + 3 stays in flight across the barrier) and meets the others at the one raw
// s_barrier -- behind which the next MFMAs can issue at once.  The memory instructions of a k-step are issued BETWEEN its
// MFMAs (one per TM MFMAs), not in front of them.  Measured on the way (tools/tile_probe.cpp, M = 2048, K = 2048, N = 4096,
// two problems): two stages + fragments read after the barrier 0.77 of the fp32 matrix peak; fragments read a k-step
// ahead 0.81; LDS-DMA 0.83; the issue order 0.90 (profiles/r05_tile_kernel_diag.txt).
// TM = 4: 128 x 128 tiles (a wave owns 64 x 64), M >= 1024 rows of the FF projections.  TM = 2: 64 x 64 tiles (a wave owns
// 32 x 32) for the 256-wide projections, whose 128-tiles would not fill the chip.
template <int TM>
struct TileFrags {
    f32x4 a[TM], b[TM];
};

__device__ __forceinline__ void glds16(const float* g, float* l)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// CONV (TM = 2, round 6): the 3 x 3 convolutions of the 2-D res-block (modules/modules.py:126-164) as an implicit GEMM on
// this kernel: K = (tap, channel) = 9 x 256, a 64-row tile is exactly one sample's 8 x 8 tokens, and the A row a thread
// fetches for k-tile kt is its own token shifted by the tap of that k-tile -- or the 64 zero bytes of `a.zero` when the tap
// leaves the image (zero padding; LDS-DMA cannot mask a lane, it can be pointed somewhere else).  The tap of a k-tile is
// scalar arithmetic on the loop counter, the select two vector instructions per k-step: no branch in the K loop.  Round 5
// ran these two launches on the skinny kernel, one tap per K slice: 9 216 workgroups that each re-read a 64 x 256 X tile
// for 16 output columns, 64.5 us per launch at B = 32 (0.48 of the fp32 matrix peak).
template <bool GEGLU, int TM, bool CONV = false>
__global__ __launch_bounds__(256, 2) void linear_tile_kernel(const TileArgs a)
{
    static_assert(TM == 2 || TM == 4, "64 x 64 or 128 x 128 tiles");
    static_assert(!GEGLU || TM == 4, "the GEGLU column pairing is laid out for 128-column tiles");
    static_assert(!CONV || (TM == 2 && !GEGLU), "the implicit-GEMM convolution walks one sample (64 tokens) per tile");
    constexpr int T = 32 * TM;          // tile rows = tile columns
    constexpr int HALF = T * 16;        // floats of one operand tile [T][16]
    constexpr int STAGE = 2 * HALF;     // [A | B]
    constexpr int NP = TM / 2;          // 1 KiB pieces per wave, operand and k-step
    // ONE LDS object (a second one beside an LDS-DMA target makes hipcc drain the DMA before every ds_read)
    __shared__ __attribute__((aligned(1024))) float smem[4 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kMaxProb; ++i)
        if (i < a.nprob && (int)blockIdx.x >= a.p[i].tile0) pi = i;
    const LinProb pr = a.p[pi];
    const int tile = (int)blockIdx.x - pr.tile0;
    const int m0 = blockIdx.y * T;
    AHV_ENC_STAMP(0);
    const int r16 = lane & 15, kq = lane >> 4;
    // staging: thread -> (row = tid / 4 (+64), 16-byte chunk = tid % 4) of both tiles
    const int srow = tid >> 2, sch = tid & 3;
    const float* xg[NP];
    const float* wg[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int j = srow + 64 * i;  // tile row
        xg[i] = pr.X + (long)(m0 + j) * a.ldx + (long)blockIdx.z * a.K + 4 * sch;
        int wrow;
        if (GEGLU) wrow = ((j >> 5) & 1) * a.geglu_h + tile * 64 + 32 * (j >> 6) + (j & 31);
        else wrow = tile * T + j;
        wg[i] = pr.W + (long)wrow * a.ldw + (long)blockIdx.z * a.K + 4 * sch;
    }
    f32x4 acc[TM][TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = a.K / 16;
    const int soff = srow * 16 + 4 * sch;                        // this thread's 16 bytes of a piece (= 4 tid floats)
    const int foffa = (16 * TM * wr + r16) * 16 + 4 * kq;        // fragment rows of this lane (+ 16 rows per i)
    const int foffb = HALF + (16 * TM * wc + r16) * 16 + 4 * kq;
    // CONV: this thread's token (y, x) inside the sample and the sample's first row
    const int cty = srow >> 3, ctx = srow & 7;
    const float* xs = pr.X + (long)m0 * 256 + 4 * sch;
    const int zoff = CONV ? (int)((a.zero + 4 * sch) - xs) : 0;   // the zero line, as an offset from this thread's row base
    auto gload = [&](int kt, int st) {  // tile kt -> stage st, 2 NP pieces of 1 KiB per wave
        float* dst = smem + st * STAGE + soff;
        if constexpr (CONV) {
            const int kg = (int)blockIdx.z * a.K + 16 * kt;   // uniform: the k-tile's first column in (tap, channel) order
            const int tap = kg >> 8, ci = kg & 255;
            const int t3 = (tap * 11) >> 5;                   // tap / 3 for tap < 9
            const int dy = t3 - 1, dx = tap - 3 * t3 - 1;
            const int ny = cty + dy, nx = ctx + dx;
            // an arithmetic select on a 32-bit offset (the workspace is far below 8 GB): written as `inside ? p : q` on pointers
            // hipcc turned the k-step into exec-masked blocks, i.e. a K loop of several basic blocks -- and then waits for
            // every DMA and fragment read in front of the MFMAs (tests/test_isa_hazard.py checks the loop's shape)
            const int keep = -(int)((unsigned)(ny | nx) < 8u);   // all ones inside the image (a negative coordinate sets the OR's sign bit)
            const int off = (((ny * 8 + nx) * 256 + ci) & keep) | (zoff & ~keep);
            glds16(xs + off, dst);
            glds16(wg[0] + 16 * kt, dst + HALF);
        } else {
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                glds16(xg[i] + 16 * kt, dst + 1024 * i);
                glds16(wg[i] + 16 * kt, dst + HALF + 1024 * i);
            }
        }
    };
    auto fread = [&](TileFrags<TM>& f, int st) {
        const float* src = smem + st * STAGE;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            f.a[i] = *reinterpret_cast<const f32x4*>(src + foffa + 256 * i);
            f.b[i] = *reinterpret_cast<const f32x4*>(src + foffb + 256 * i);
        }
    };
    auto mma = [&](const TileFrags<TM>& f) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[i][s4], f.b[j][s4], acc[i][j], 0, 0, 0);
    };
    // vmcnt(TM) lgkmcnt(0): this wave's pieces of tile kt + 2 are in LDS, the TM pieces of tile kt + 3 may still be on
    // their way when the barrier is met; `nxt` has long arrived
    constexpr int kWait = 0x0070 | TM;
    // one k-step: `cur` holds tile kt's fragments, `nxt` receives tile kt + 1's; tile kt + 3 goes into the stage tile
    // kt - 1 occupied (its fragments were read two barriers ago).  No conditions in here: behind the last tile the loads
    // repeat tile nk - 1 into a stage nobody reads again and the fragment read fetches a tile nobody multiplies -- every
    // branch would cost hipcc its count of what is in flight (it then waits for the fragment reads in front of the MFMAs).
    auto kstep = [&](int kt, const TileFrags<TM>& cur, TileFrags<TM>& nxt) {
        __builtin_amdgcn_sched_barrier(0);
        gload(kt + 3 < nk ? kt + 3 : nk - 1, (kt + 3) & 3);
        fread(nxt, (kt + 1) & 3);
        mma(cur);
        // issue order: the 3 TM memory instructions go BETWEEN the MFMAs (one per TM), where their issue slots are free --
        // all of them in front of the first MFMA leave the matrix pipe waiting whenever the SIMD's other wave stands at
        // the same point
#pragma unroll
        for (int g = 0; g < TM; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, TM, 0);  // TM MFMAs
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);   // 1 VMEM (an LDS-DMA piece)
        }
#pragma unroll
        for (int g = 0; g < 2 * TM; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, TM, 0);  // TM MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // 1 DS read
        }
        __builtin_amdgcn_sched_group_barrier(0x008, TM * TM, 0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(kWait);
        __builtin_amdgcn_s_barrier();
    };
    // prologue: tiles 0, 1, 2 requested; tiles 0 and 1 landed before the first barrier
    TileFrags<TM> f0, f1;
    gload(0, 0);
    gload(1, 1);
    gload(nk > 2 ? 2 : nk - 1, 2);
    __builtin_amdgcn_s_waitcnt(kWait);
    __builtin_amdgcn_s_barrier();
    AHV_ENC_STAMP(1);
    fread(f0, 0);
    // (a wait here, or hipcc carries "f0 pending" into the loop)
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    for (int kt = 0; kt < nk; kt += 2) {  // nk is even (launch_linear: K per split is a multiple of 32)
        kstep(kt, f0, f1);
        kstep(kt + 1, f1, f0);
    }
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0): the repeated loads have landed before the LDS is given up
    AHV_ENC_STAMP(4);
    // D layout: acc[i][j][r] = C[m0 + 16 TM wr + 16 i + 4 kq + r][column 16 TM wc + 16 j + r16 of the tile]: 4-byte stores, four
    // 64-byte row segments per instruction.  (The transposed tiles -- W rows as the A operand, a lane then holds four
    // consecutive columns and stores 16 bytes, sixteen 64-byte row segments per instruction -- measured 1-3 % SLOWER.)
    if constexpr (GEGLU) {
        const int H = a.geglu_h;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = tile * 64 + 32 * wc + 16 * j + r16;
            const float bv = pr.bias[col], bg = pr.bias[H + col];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const long row = m0 + 64 * wr + 16 * i + 4 * kq + r;
                    const f32x2 y = geglu_pk(f32x2{acc[i][j][r] + bv, acc[i][j][r + 1] + bv},
                                             f32x2{acc[i][j + 2][r] + bg, acc[i][j + 2][r + 1] + bg});
                    __builtin_nontemporal_store(y[0], pr.P + row * H + col);
                    __builtin_nontemporal_store(y[1], pr.P + (row + 1) * H + col);
                }
        }
    } else {
        float* P = pr.P + (long)blockIdx.z * a.M * pr.N;  // split-K slab [ks][M][N]
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int col = tile * T + 16 * TM * wc + 16 * j + r16;
            const float bias = (pr.bias != nullptr && gridDim.z == 1) ? pr.bias[col] : 0.0f;  // a bias only without split-K (host)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    __builtin_nontemporal_store(acc[i][j][r] + bias, P + (long)(m0 + 16 * TM * wr + 16 * i + 4 * kq + r) * pr.N + col);
        }
    }
    AHV_ENC_STAMP(6);
}

}  // namespace ahv
