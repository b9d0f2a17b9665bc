// ahv_split.h -- GEMM1 and GEMM2 of the fused scorer on the f16 matrix pipe with split operands (OPT-IN per call through
// AHV_SCORE_SPLIT_F16: the default stays the all-fp32 dual kernel).
//
// Why: fp32 MFMA tops out at 157 TFLOP/s and shares its issue slots with VALU work (ahv_dual.h), so the
// fp32 kernel sits at ~80 % of a roofline that is itself 16x below the f16 matrix pipe.  Each fp32
// operand x is written as hi + lo with hi = x truncated to 11 significant bits and lo = x - hi rounded
// to f16; the three products hi*hi + hi*lo + lo*hi are accumulated in fp32 by v_mfma_f32_16x16x32_f16
// (hi*hi is exact in fp32, the dropped lo*lo term is 2^-22 relative).  Measured against the fp32
// oracle the scores agree to ~1e-6, two orders inside the 1e-4 parity bar (tests/test_gpu_split.py), but
// the arithmetic is NOT IEEE fp32 -- hence opt-in.  Operands are prescaled by powers of two taken from their
// largest magnitude (split_prescale_exp), so any finite fp32 range works.
//
// K order inside a slab is (spatial index, channel) with the channel fastest: a lane's own 16 blended
// channels are then two complete B fragments, the gather stores them with four ds_write_b128 and ONE
// image serves all three slab views with plain ds_read_b128.
//
// v_mfma_f32_16x16x32_f16: A[row = lane&15][k = 8*(lane>>4) + j], B[k = 8*(lane>>4) + j][col = lane&15],
// D[row = 4*(lane>>4) + reg][col = lane&15]  (j = 0..7, the eight halfs of the operand register quad).
#pragma once
#include "ahv_device.h"
#include "ahv_dual.h"

namespace ahv {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Both operands are prescaled by a power of two chosen from their largest magnitude (per launch for W1,
// per sample for the source volume) so that max |x| * 2^e lies in [2^13, 2^14): hi never overflows f16 and
// lo stays a normal f16 for everything within 2^-13 of the maximum.  The exact 2^-(eW+eV) comes back out
// through the GEMM2 A operand.
__device__ __forceinline__ int split_prescale_exp(float amax)
{
    if (!(amax > 0.0f) || amax > 3.0e38f) return 0;  // all-zero, NaN or inf operands: nothing to gain
    int ex;
    (void)frexpf(amax, &ex);  // amax = m * 2^ex, m in [0.5, 1)
    const int e = 14 - ex;
    return e < -60 ? -60 : (e > 60 ? 60 : e);
}

// max over the workgroup; `scratch` = 8 floats of LDS nobody else is using right now
__device__ __forceinline__ float block_absmax(float x, float* scratch, int tid)
{
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) x = fmaxf(x, __shfl_xor(x, sft, 64));
    if ((tid & 63) == 0) scratch[tid >> 6] = x;
    __syncthreads();
    float m = scratch[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) m = fmaxf(m, scratch[i]);
    __syncthreads();
    return m;
}
constexpr int kSplitTableFrags = 48;       // 12 groups (slab, k-step) x {m0 hi, m0 lo, m1 hi, m1 lo}
constexpr int kSplitTableBytes = kSplitTableFrags * 64 * 16;  // 48 KiB
// Registers: this kernel is bound by LDS THROUGHPUT (every latency knob is flat: request-ring depths 1 to 7 and GEMM operand
// requests 1 to 3 k-steps ahead all time the same, profiles/r04v_split_lds_traffic.txt), so the ring runs at depth 2 and
// the 64 registers that frees hold five of the eight W1 fragment groups every quarter reads (x slab k-steps 0-3, y slab
// k-step 0): 80 of a hypothesis' 144 W1 fragment reads never reach the LDS.  Measured per resident group: -0.9 % of kernel
// time (0.3588 -> 0.3439 ms for the five on one box).
constexpr int kSplitHatDepth = 2;
constexpr int kSplitResident = 5;
constexpr int kSplitImageBytes = 128 * 64;  // per wave: 128 voxels x (16 hi + 16 lo halfs), as two planes

// ---- W1 fragment table -----------------------------------------------------------------
// Group G = 4*s + ks (s = slab x,y,z; ks = k-step of 32), fragment i = 2*m + part at f16x8 slot
// (4*G + i)*64 + lane.  Lane (row, kq), half j holds
//   W1[16m + row][128 s + c*8 + idx],  idx = 2 ks + (kq >> 1),  c = 8 (kq & 1) + j
// i.e. k = idx*16 + c inside the slab; for the z slab idx = a, so k-step ks = the quarter.
__device__ __forceinline__ void stage_w1_split(f16x8* table, const float* __restrict__ W1, float scale, int tid, int nthreads)
{
    for (int i = tid; i < kSplitTableFrags * 64; i += nthreads) {
        const int lane = i & 63, frag = i >> 6;
        const int G = frag >> 2, m = (frag >> 1) & 1, part = frag & 1;
        const int s = G >> 2, ks = G & 3;
        const int row = lane & 15, kq = lane >> 4;
        const float* w = W1 + (16 * m + row) * 384 + 128 * s + 2 * ks + (kq >> 1);
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = w[(8 * (kq & 1) + j) * 8] * scale;
            const _Float16 hi = (_Float16)x;
            v[j] = part ? (_Float16)(x - (float)hi) : hi;
        }
        table[i] = v;
    }
}

// Source volume -> LDS, prescaled per sample; returns the exponent used (512 threads, 16 values each).
// `bad` (per thread): one of this thread's voxels is NaN / inf.  Such a sample is not scaled (the maximum is taken to be
// inf -- v_max would DROP a NaN) and leaves the split arithmetic for the exact fp32 path (ahv_exact.h), which reads this image.
__device__ __forceinline__ int stage_src_volume_scaled(float* srcT, const float* __restrict__ vol, float* scratch, int tid, bool& bad)
{
    float x[16];
    float m = 0.0f;
    bad = false;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        x[k] = vol[tid + 512 * k];
        m = fmaxf(m, fabsf(x[k]));
        bad = bad || __builtin_amdgcn_classf(x[k], 0x207);  // sNaN | qNaN | -inf | +inf
    }
    if (bad) m = __builtin_inff();
    const int e = split_prescale_exp(block_absmax(m, scratch, tid));
    const float scale = ldexpf(1.0f, e);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = tid + 512 * k, c = i >> 9, v = i & 511;
        srcT[((v >> 6) * kSrcPlaneRows + ((v >> 3) & 7) * kSrcRowsY + (v & 7)) * kSrcStride + c] = x[k] * scale;
    }
    return e;
}

// The exact path (ahv_exact.h) multiplies the source image by the UNSCALED head weights from global memory and never
// undoes the prescales: when it is the WEIGHTS that are non-finite while the volume is finite, the image above holds the
// volume times 2^e and the pre-activations that stay finite (W1 = -inf against positive voxels: -inf, ReLU'd to 0) come
// out against a bias that is 2^e too small.  Such a sample is staged again as it is (rare path, uniform branch).
__device__ __forceinline__ void restage_src_volume_unscaled(float* srcT, const float* __restrict__ vol, int tid)
{
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = tid + 512 * k, c = i >> 9, v = i & 511;
        srcT[((v >> 6) * kSrcPlaneRows + ((v >> 3) & 7) * kSrcRowsY + (v & 7)) * kSrcStride + c] = vol[i];
    }
}

// ---- rotated quarter image ---------------------------------------------------------------
// Two planes of 4 KB per wave: the hi halves and, 4 096 bytes on, the lo halves.  Inside a plane voxel (a0, b, e) of the
// quarter owns the 32-byte row a0 + 2e + 16b = [c0-7 | c8-15]; the 16-byte slot of a chunk inside its 256-byte LDS line
// is address bits 4-7 = (chunk, row & 7), and those four bits are XORed with voxel bits:
//     bit 4 ^= a0      bit 5 ^= e2      bit 6 ^= b0      bit 7 ^= b1
// (bits 5-7 = a0, e0, e1 of the row are XORed with OTHER bits only, so the map stays one to one; b >> 2 is the gather's
// pass and stays out, so pass 1 is "+ 2 048 bytes"; lo is "+ 4 096 bytes": both ride in the instructions' offset fields).
// What the swizzle has to satisfy (MI355X_MICROARCH.md, LDS): a ds_read_b128 is served in four groups of 16 lanes
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, + 32), one cycle each if the 16 lanes hit 16 different slots of the 256-byte
// line; a ds_write_b128 in eight groups of 8 CONTIGUOUS lanes over 128 bytes (slot = address bits 4-6).  Round 3's image
// (64-byte rows [hi | lo], the chunk bits XORed only) had its stores 2-way (256 extra cycles per hypothesis) and the
// x- and z-slab fragment reads 2-way (128 each): 512 of the 1 167 conflict cycles SQ_LDS_BANK_CONFLICT counted per
// hypothesis, the other 655 being the gather's.  tools/split_image_sim.py models both group shapes -- it reproduces the
// counter for round 3's layout, and for a first attempt of this round that used the read groups for the stores (768 +
// 655 = the 1 423 measured) -- and enumerates the GF(2)-linear swizzles: 12 288 are conflict-free for the 32 stores
// (plain and mirrored quarters, both passes) and the 96 fragment reads of a hypothesis; this one has the fewest terms.
// Measured with 64-byte rows and an equivalent swizzle, binaries alternating on one box: conflict cycles 1 167 -> 655 per
// hypothesis (0.339 -> 0.223 of the LDS cycles), 0.3770 -> 0.3688 ms (profiles/r04m_split_swizzle_ab.txt); the planes
// then take the lo addresses (lo was "address ^ 32": one register per fragment address) out of the register file.
constexpr int kSplitLoPlane = 4096, kSplitPass = 2048;
__device__ __forceinline__ int split_addr(int a0, int b, int e, int chunk)  // chunk 0 / 1 = channels 0-7 / 8-15 (hi plane)
{
    const int x = a0 | ((e >> 2) << 1) | ((b & 3) << 2);
    return ((a0 + 2 * e + 16 * b) * 32 + (chunk << 4)) ^ (x << 4);
}

__device__ __forceinline__ unsigned pk_rtz(float a, float b)
{
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
}

// hi = (x0, x1) rounded towards zero to f16 = their top 11 significant bits; lo = x - hi exactly (then rounded to f16), each
// difference on ONE instruction that reads its f16 operand in place (v_fma_mix_f32: fma(f16 -> f32, -1, x)) -- four
// instructions per pair of values where masking x, subtracting and converting took six (five with a packed subtraction):
// 1 336 -> 1 192 vector instructions per hypothesis, -1.5 % of kernel time.  hipcc has no pattern for it (it converts and
// subtracts): op_sel_hi marks source 0 as f16, op_sel picks its half.  (v_fma_mixlo_f16 / mixhi_f16 would write the lo pair
// directly, three instructions per pair: measured 0.6 % SLOWER -- the second writes into the register of the first.)
// The op_sel here picks a 16-bit half of an f16 source; it is not the packed-fp32 cross-half read of the hazard low_half
// guards against, and the forced-gap and fresh-process tests of tests/test_gpu_split.py run through these instructions.
__device__ __forceinline__ unsigned split_hi_lo(unsigned& lo, float x0, float x1)
{
    const unsigned h = pk_rtz(x0, x1);
    float l0, l1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(h), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(h), "v"(x1));
    lo = pk_rtz(l0, l1);
    return h;
}

// The gather is the fp32 kernel's (ahv_dual.h: hat weights on a clamped base row, one base address per voxel, a
// request ring six rows deep, the 4 x 2 x 2-box lane map); only the store differs: the sixteen blended channels are
// split into hi (the top 11 significant bits, exactly an f16 in the normal range) and lo (the rest) and leave as
// 16-byte stores, conflict-free under the image's swizzle (split_addr above).
struct SplitDst {
    int chunk[2];    // byte offsets of [hi c0-7 | hi c8-15] of the lane's pass-0 voxel (pass 1: + kSplitPass; lo: + kSplitLoPlane)
    int chunk_m[2];  // the same for the lane's voxel in a MIRRORED quarter, (7 - x, 7 - y, 1 - z) (hat_mirror, ahv_dual.h)
};

__device__ __forceinline__ SplitDst split_dst(int lane)
{
    const LaneVox lv = lane_vox(lane);
    SplitDst d;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        d.chunk[c] = split_addr(lv.a0, lv.bq, lv.e, c);  // b = 4 p + bq: the pass keeps b & 3
        d.chunk_m[c] = split_addr(1 - lv.a0, 3 - lv.bq, 7 - lv.e, c);
    }
    asm volatile("" : "+v"(d.chunk[0]), "+v"(d.chunk[1]));
    asm volatile("" : "+v"(d.chunk_m[0]), "+v"(d.chunk_m[1]));
    return d;
}

template <bool MIR>
struct HatStoreSplit {
    static constexpr bool kXdlKernel = true;  // GEMM1 runs on XDL MFMAs here: broadcast scalars stay in low halves (low_half, ahv_dual.h)
    static constexpr int kDepth = kSplitHatDepth;
    char* img;
    SplitDst d;
    __device__ __forceinline__ void operator()(int p, const f32x2 (&o)[8]) const
    {
        // eight channels at a time, each half stored before the next is converted: the request ring of the other pass
        // is live here and sixteen conversion temporaries on top of it do not fit in 256 registers
        char* dst = img + p * kSplitPass;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            unsigned hi[4], lo[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // scalars first: __builtin_bit_cast applied to a vector ELEMENT expression reads element 0 with this
                // hipcc (ROCm 7.2) whatever the index
                const float x0 = o[4 * half + i][0], x1 = o[4 * half + i][1];
                hi[i] = split_hi_lo(lo[i], x0, x1);
            }
            *reinterpret_cast<u32x4*>(dst + (MIR ? d.chunk_m[half] : d.chunk[half])) = u32x4{hi[0], hi[1], hi[2], hi[3]};
            *reinterpret_cast<u32x4*>(dst + kSplitLoPlane + (MIR ? d.chunk_m[half] : d.chunk[half])) = u32x4{lo[0], lo[1], lo[2], lo[3]};
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

// the 16 blend steps of a quarter whose prologue (hat_prologue, ahv_dual.h) has been issued
template <bool MIR = false>
__device__ __forceinline__ void hat_body_split(HatState& st, char* img, const SplitDst& dst)
{
    f32x2 o[8];
    const HatStoreSplit<MIR> store = {img, dst};
    __builtin_amdgcn_s_setprio(1);
    HatSteps<0, HatStoreSplit<MIR>, MIR>::run(st, o, store);
    __builtin_amdgcn_s_setprio(0);
}

// ---- GEMM1 on one quarter: 72 x v_mfma_f32_16x16x32_f16 -----------------------------------------
#define AHV_MFMA_F16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16((A), (B), (C), 0, 0, 0)

// Operands of one k-step.  Steps 0-3 = x slab (ks), 4-7 = y slab (ks), 8-11 = z slab (tile t).
struct SplitStep {
    f16x8 bh, bl;    // B fragment pair of the step
    f16x8 a[4];      // {m0 hi, m0 lo, m1 hi, m1 lo}; the z steps share one quad
};

// the W1 fragment groups 0 .. kSplitResident-1, in registers for the whole launch
struct SplitResident {
    f16x8 g[kSplitResident][4];
};
__device__ __forceinline__ void split_load_resident(SplitResident& r, const f16x8* table, int lane)
{
#pragma unroll
    for (int G = 0; G < kSplitResident; ++G)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r.g[G][i] = table[(4 * G + i) * 64 + lane];
            asm volatile("" : "+v"(r.g[G][i]));
        }
}

template <int Q, int S>
__device__ __forceinline__ void split_load(SplitStep& o, const SplitResident& res, const f16x8* T, const char* img, int i0, int j, int kh, int kc)
{
    constexpr int ks = S & 3;
    int off;
    if (S < 4) off = split_addr(i0, j, 2 * ks + kh, kc);        // position (a0 = i0, b = j), k = (e, c)
    else if (S < 8) off = split_addr(i0, 2 * ks + kh, j, kc);   // position (a0 = i0, e = j), k = (b, c)
    else off = split_addr(kh, 2 * ks + i0, j, kc);              // position (b = 2t + i0, e = j), k = (a0, c)
    o.bh = *reinterpret_cast<const f16x8*>(img + off);
    o.bl = *reinterpret_cast<const f16x8*>(img + off + kSplitLoPlane);
    if (S <= 8) {
        constexpr int G = S < 4 ? ks : (S < 8 ? 4 + ks : 8 + Q);
#pragma unroll
        for (int i = 0; i < 4; ++i) o.a[i] = (G < kSplitResident) ? res.g[G < kSplitResident ? G : 0][i] : T[(4 * G + i) * 64];
    }
}

// Stress knob of tools/first_launch.cpp, never set in the product (tests/test_gpu_split.py builds first_launch with it as the
// regression test of low_half): AHV_DIAG_MFMA_GAP="s_nop 7" leaves the matrix pipe idle
// between any two MFMAs, which is what exposes the packed-fp32 op_sel hazard (low_half, ahv_dual.h) on every hypothesis
// instead of on the few that meet an instruction-fetch stall in a process' first launch.
#ifdef AHV_DIAG_MFMA_GAP
#define AHV_MFMA_GAP __builtin_amdgcn_sched_barrier(0); asm volatile(AHV_DIAG_MFMA_GAP ::: "memory"); __builtin_amdgcn_sched_barrier(0);
#else
#define AHV_MFMA_GAP
#endif
template <int Q, int S>
__device__ __forceinline__ void split_mfma(f32x4 (&acc)[2][4], const SplitStep& o, const f16x8 (&az)[4])
{
    constexpr int t = S < 8 ? Q : (S & 3);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const f16x8 ah = S < 8 ? o.a[2 * m] : az[2 * m], al = S < 8 ? o.a[2 * m + 1] : az[2 * m + 1];
        acc[m][t] = AHV_MFMA_F16(al, o.bh, acc[m][t]);
        AHV_MFMA_GAP
        acc[m][t] = AHV_MFMA_F16(ah, o.bl, acc[m][t]);
        AHV_MFMA_GAP
        acc[m][t] = AHV_MFMA_F16(ah, o.bh, acc[m][t]);
        AHV_MFMA_GAP
    }
}

// Twelve k-steps, software-pipelined by hand: the operands of step S + kSplitAhead are requested before the six MFMAs of
// step S are issued, and sched_barrier keeps the compiler from hoisting every load of the quarter to the top (which costs
// ~100 registers and spills).  `hook` runs once, ahead of the MFMAs of step 8 (a gather prologue, as in gemm1_quarter_pipe).
constexpr int kSplitAhead = 1;  // 2 and 3 measured the same (round 4)
template <int Q, int S>
struct SplitSteps {
    template <typename Hook>
    static __device__ __forceinline__ void run(f32x4 (&acc)[2][4], SplitStep (&s)[kSplitAhead + 1], f16x8 (&az)[4], const SplitResident& res, const f16x8* T,
                                               const char* img, int i0, int j, int kh, int kc, Hook hook)
    {
        if (S + kSplitAhead < 12) {
            constexpr int L = S + kSplitAhead < 12 ? S + kSplitAhead : 0;
            split_load<Q, L>(s[L % (kSplitAhead + 1)], res, T, img, i0, j, kh, kc);
            if (L == 8) { az[0] = s[L % (kSplitAhead + 1)].a[0]; az[1] = s[L % (kSplitAhead + 1)].a[1]; az[2] = s[L % (kSplitAhead + 1)].a[2]; az[3] = s[L % (kSplitAhead + 1)].a[3]; }
        }
        if (S == 8) hook();
        __builtin_amdgcn_sched_barrier(0);
        split_mfma<Q, S>(acc, s[S % (kSplitAhead + 1)], az);
        __builtin_amdgcn_sched_barrier(0);
        SplitSteps<Q, S + 1>::run(acc, s, az, res, T, img, i0, j, kh, kc, hook);
    }
};
template <int Q>
struct SplitSteps<Q, 12> {
    template <typename Hook>
    static __device__ __forceinline__ void run(f32x4 (&)[2][4], SplitStep (&)[kSplitAhead + 1], f16x8 (&)[4], const SplitResident&, const f16x8*, const char*, int, int,
                                               int, int, Hook) {}
};

template <int Q, typename Hook>
__device__ __forceinline__ void gemm1_quarter_split(f32x4 (&acc)[2][4], const SplitResident& res, const f16x8* table, const char* img,
                                                    int lane, Hook hook)
{
    const int n = lane & 15, kq = lane >> 4;
    const int i0 = n >> 3, j = n & 7, kh = kq >> 1, kc = kq & 1;
    const f16x8* T = table + lane;
    SplitStep s[kSplitAhead + 1];
    f16x8 az[4];
    split_load<Q, 0>(s[0], res, T, img, i0, j, kh, kc);
    if (kSplitAhead > 1) split_load<Q, 1>(s[1], res, T, img, i0, j, kh, kc);
    if (kSplitAhead > 2) split_load<Q, 2>(s[2 % (kSplitAhead + 1)], res, T, img, i0, j, kh, kc);
    SplitSteps<Q, 0>::run(acc, s, az, res, T, img, i0, j, kh, kc, hook);
}

// ---- GEMM2 on the XDL pipe -----------------------------------------------------------------------
// v = W2 relu(u) + b2 is 64 fp32 MFMAs per hypothesis in the fp32 formulation: 2 048 cycles during which the SIMD issues
// nothing else, where the whole of GEMM1 is 4 608 XDL cycles (skipping GEMM2 altogether, as a bound: 0.362 -> 0.338 ms
// per 50 000 hypotheses, profiles/r04v_split_lds_traffic.txt).  Here it is 24 v_mfma_f32_16x16x32_f16 on hi/lo halves
// like GEMM1.  No data moves between lanes: the contraction index of a 16x16x32 fragment is (kq = lane >> 4, j = 0..7), a
// lane's GEMM1 accumulators acc[m][t][r] ARE rows 16 m + 4 kq + r of the activations at position 16 t + (lane & 15), so with
//     feature(kq, j) = 16 (j >> 2) + 4 kq + (j & 3)
// the B fragment of tile t is the lane's own {acc[0][t][0..3], acc[1][t][0..3]} and the A fragments are W2 with its
// columns taken in that order -- exactly the sixteen floats DualFrags::a2 holds.
// Scales: u arrives in units of 2^(eW1 + eV) (split_prescale_exp); the activations of the four positions (lane & 15)
// + 16 t are brought to a maximum in [2^13, 2^14) by a power of two of their own (the four lanes kq = 0..3 that hold them
// agree on the maximum with two v_permlane swaps; elements 2^-27 and more below that maximum lose bits -- of an absolute
// size 2^-38 of it), W2 to the same range once per launch, and the product of the three scales comes back out in the
// fused multiply-add that adds b2.
struct Split2Frags {
    f16x8 ah[2], al[2];  // [m2]: W2[16 m2 + (lane & 15)][feature(lane >> 4, j)] * 2^e2, hi and lo halves
};

__device__ __forceinline__ void split_w2_frags(Split2Frags& w, const DualFrags& f, float scale)
{
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = f.a2[j >> 2][j & 3][m2] * scale;
            const _Float16 hi = (_Float16)x;
            w.ah[m2][j] = hi;
            w.al[m2][j] = (_Float16)(x - (float)hi);
        }
}

struct Gemm2Scale {
    float pre, post;  // per lane: activations * pre before the split; MFMA sums * post + b2 behind it
};

// relu in place (as integers: a negative float is a negative integer), then one scale for the four positions
// (lane & 15) + 16 t of the lane.  exp_sum = e2 + eW1 + eV: the exponents of the three per-launch / per-sample prescales.
__device__ __forceinline__ Gemm2Scale gemm2_split_scale(f32x4 (&acc)[2][4], int exp_sum)
{
    int mt[4];  // four short chains instead of one of sixteen: this is the head of the hypothesis' tail, nothing overlaps it
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        // non-negative floats order like their bit patterns (v_max3_i32); a NaN counts as the largest exponent
        const i32x4 u0 = __builtin_elementwise_max(__builtin_bit_cast(i32x4, acc[0][t]), i32x4{0, 0, 0, 0});
        const i32x4 u1 = __builtin_elementwise_max(__builtin_bit_cast(i32x4, acc[1][t]), i32x4{0, 0, 0, 0});
        acc[0][t] = __builtin_bit_cast(f32x4, u0);
        acc[1][t] = __builtin_bit_cast(f32x4, u1);
        const int a = __builtin_elementwise_max(__builtin_elementwise_max(u0[0], u0[1]), u0[2]);
        const int b = __builtin_elementwise_max(__builtin_elementwise_max(u1[0], u1[1]), u1[2]);
        mt[t] = __builtin_elementwise_max(__builtin_elementwise_max(a, b), __builtin_elementwise_max(u0[3], u1[3]));
    }
    int mx = __builtin_elementwise_max(__builtin_elementwise_max(mt[0], mt[1]), __builtin_elementwise_max(mt[2], mt[3]));
    {   // maximum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 that hold these positions: v_permlane32_swap(a, b)
        // exchanges lanes 32-63 of a with lanes 0-31 of b, so with a = b every lane sees its partner's value
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)mx, (unsigned)mx, false, false);
        mx = __builtin_elementwise_max((int)r[0], (int)r[1]);
        const auto q = __builtin_amdgcn_permlane16_swap((unsigned)mx, (unsigned)mx, false, false);
        mx = __builtin_elementwise_max((int)q[0], (int)q[1]);
    }
    int s = (int)(((unsigned)mx >> 23) & 255u) - (127 + 13);  // the maximum in [2^13, 2^14) after the scaling
    s = s < -100 ? -100 : (s > 100 ? 100 : s);                // (all zero: any s will do)
    int e = s - exp_sum;
    e = e < -126 ? -126 : (e > 127 ? 127 : e);
    return {__uint_as_float((unsigned)(127 - s) << 23), __uint_as_float((unsigned)(127 + e) << 23)};
}

// position tile t: u0 = relu(acc[0][t]), u1 = relu(acc[1][t]) in, the lane's 2 x 4 output channels out
__device__ __forceinline__ void gemm2_split_tile(f32x4& v0, f32x4& v1, const f32x4& u0, const f32x4& u1, const Split2Frags& w,
                                                 const f32x4 (&bias)[2], const Gemm2Scale& sc)
{
    // the two scales stay in low halves of their own (low_half, ahv_dual.h: no op_sel read of a high half next to XDL MFMAs)
    const float pre = low_half(sc.pre), post = low_half(sc.post);
    unsigned hi[4], lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // scale, split (as the gather's store does: hi = the top 11 significant bits, lo = the rest)
        const f32x4& u = (i >> 1) ? u1 : u0;
        const f32x2 x = f32x2{u[2 * (i & 1)], u[2 * (i & 1) + 1]} * f32x2{pre, pre};
        // scalars first: __builtin_bit_cast applied to a vector ELEMENT expression reads element 0 with this hipcc
        // (ROCm 7.2) whatever the index
        const float x0 = x[0], x1 = x[1];
        hi[i] = split_hi_lo(lo[i], x0, x1);
    }
    const f16x8 bh = __builtin_bit_cast(f16x8, u32x4{hi[0], hi[1], hi[2], hi[3]});
    const f16x8 bl = __builtin_bit_cast(f16x8, u32x4{lo[0], lo[1], lo[2], lo[3]});
    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
    d0 = AHV_MFMA_F16(w.al[0], bh, d0);
    d1 = AHV_MFMA_F16(w.al[1], bh, d1);
    d0 = AHV_MFMA_F16(w.ah[0], bl, d0);
    d1 = AHV_MFMA_F16(w.ah[1], bl, d1);
    d0 = AHV_MFMA_F16(w.ah[0], bh, d0);
    d1 = AHV_MFMA_F16(w.ah[1], bh, d1);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const f32x2 r0 = __builtin_elementwise_fma(f32x2{d0[2 * hh], d0[2 * hh + 1]}, f32x2{post, post}, f32x2{bias[0][2 * hh], bias[0][2 * hh + 1]});
        const f32x2 r1 = __builtin_elementwise_fma(f32x2{d1[2 * hh], d1[2 * hh + 1]}, f32x2{post, post}, f32x2{bias[1][2 * hh], bias[1][2 * hh + 1]});
        v0[2 * hh] = r0[0]; v0[2 * hh + 1] = r0[1];
        v1[2 * hh] = r1[0]; v1[2 * hh + 1] = r1[1];
    }
}

}  // namespace ahv
