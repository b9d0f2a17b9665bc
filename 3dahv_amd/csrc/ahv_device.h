// ahv_device.h -- device-side building blocks shared by the fused scorer and the
// op-level kernels (gfx950 / CDNA4 only: wave64, fp32 MFMA 16x16x4, 160 KiB LDS).
//
// Geometry (fixed by the reference): volume V[c][d][h][w], c<16, d,h,w<8
// (modules/modules.py:64,97); head GEMM K = 3*16*8 = 384 -> 32 channels at 64
// positions (modules/modules.py:66-70,112-124).
//
// Work decomposition: ONE WAVE OWNS ONE HYPOTHESIS.  It produces the rotated volume a QUARTER at a time
// (d in {2q,2q+1}: 128 voxels x 16 ch = 8 KiB) into a private LDS buffer and contracts that quarter against W1
// with v_mfma_f32_16x16x4_f32.  Waves never synchronise with each other inside the hypothesis loop: no s_barrier
// on the hot path.  (Where W1 lives -- LDS fragment table, two waves per SIMD -- is ahv_dual.h; the kernels that
// kept it in 192 registers at one wave per SIMD are retired: git history, round 1.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>


namespace ahv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- LDS images -------------------------------------------------------------
// Source volume, channel-last, one 80-byte row per voxel (16 ch + 4 pad floats):
// a trilinear corner is four ds_read_b128; the 80-B stride maps voxel v, chunk k
// to 16-B slot (5v + k) mod 16, which spreads neighbouring voxels over all slots.
constexpr int kSrcStride = 20;
// Row index = kSrcPlaneRows z + kSrcRowsY y + x with (9, 76): the 16-B slot of a row is 5 (x + 9 y + 76 z) mod 16,
// i.e. (x + 9 y + 12 z) mod 16 up to the unit 5.  A ds_read_b128 is served in four groups of 16 lanes
// ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32: MI355X_MICROARCH.md, LDS) and two lanes of a group
// collide when their rows differ but share a slot.  Simulated over Haar rotations with the real lane groups
// (LDS cycles per conflict-free cycle of the gather's reads):
//   dense 8 x 64 rows, x-run lane map (round 1)              3.80
//   (8, 74), x-run lane map (rounds 1-2, measured 2.44)      2.43
//   (9, 76), x-run lane map                                  2.21
//   (8, 67), 4x2x2-box lane map (lane_vox, ahv_dual.h)       1.87
//   (9, 76), 4x2x2-box lane map                              1.64   <- this build; the best linear form mod 16
// The box map makes the 16 lanes of a group a compact 4 x 2 x 2 block of output voxels, so their base rows are a
// rotated compact block too and a linear slot function separates most of them.  608 rows (47.5 KiB): all the LDS
// that is left beside the W1 table and the quarter images.
constexpr int kSrcRowsY = 9;
constexpr int kSrcPlaneRows = 76;
constexpr int kSrcFloats = 8 * kSrcPlaneRows * kSrcStride;  // 47.5 KiB
// Rotated quarter: [16 c][128] floats, the 128 voxels (a0, b, e) of a plane XOR-
// swizzled so that all three slab read patterns AND the producer's writes are
// ds_*_b32 bank-conflict free (bank = addr mod 32 per 32-lane half):
//   bank bits = [e0, e1^b1, e2^b2, a0, b0], bits 5,6 = b1,b2
constexpr int kQuarterFloats = 16 * 128;  // 8 KiB

__device__ __forceinline__ int qoff(int a0, int b, int e)
{
    return (e ^ (b & 6)) | (a0 << 3) | ((b & 1) << 4) | ((b >> 1) << 5);
}

// XCD-aware work assignment.  Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8 labels the
// workgroups that share an L2), while hypothesis h goes to "residue" h % G: with residue = blockIdx.x the 3.5
// rotations that share a 128-byte line of R would be fetched by workgroups on 3-4 different XCDs, i.e. from
// HBM several times (measured: 10.9 MB per launch for 1.8 MB of R).  The bijective remap below hands each
// XCD a contiguous range of residues, so neighbouring hypotheses meet in one L2.  Pure placement: any
// residue permutation is correct.
__device__ __forceinline__ int xcd_residue(int bid, int nwg, int ny)
{
    if (nwg < 16 || (ny > 1 && (nwg & 7) != 0)) return bid;  // with gy > 1 the label is (x + y*gx) % 8
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Orders a wave's own LDS writes before its later LDS reads/writes at compiler
// level.  Hardware executes one wave's DS instructions in order, so no
// instruction is needed; without this the compiler may legally hoist a lane's
// read above another lane's write (per-thread alias analysis).
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// ---- head weights as MFMA fragments ------------------------------------------
// v_mfma_f32_16x16x4_f32: A[row = lane&15][k = lane>>4], B[k = lane>>4][col = lane&15],
// D[row = 4*(lane>>4)+reg][col = lane&15].  Rows = output channels (2 m-tiles of 16),
// columns = positions (4 n-tiles of 16: tile t holds positions i in {2t,2t+1}, j<8).
struct HeadFrags {
    float ax[16][2][2];  // x slab  [c][eh][m]  : W1[16m+row][      c*8 + 4*eh + kq]   (k = w)
    float ay[16][2][2];  // y slab  [c][bh][m]  : W1[16m+row][128 + c*8 + 4*bh + kq]   (k = h)
    float az[4][8][2];   // z slab  [q][cp][m]  : W1[16m+row][256 + (2cp+(kq>>1))*8 + 2q+(kq&1)]  (k = d)
    float a2[2][4][2];   // GEMM2   [m][r][m2]  : W2[16m2+row][16m + 4kq + r]
    f32x4 bias[2];       // [m2]                : b2[16m2 + 4kq + r]
};

__device__ __forceinline__ void load_head_frags(HeadFrags& f, const float* __restrict__ W1,
                                                const float* __restrict__ W2,
                                                const float* __restrict__ b2, int lane)
{
    const int row = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const float* w = W1 + (16 * m + row) * 384;
#pragma unroll
        for (int c = 0; c < 16; ++c)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                f.ax[c][hh][m] = w[c * 8 + 4 * hh + kq];
                f.ay[c][hh][m] = w[128 + c * 8 + 4 * hh + kq];
            }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cp = 0; cp < 8; ++cp)
                f.az[q][cp][m] = w[256 + (2 * cp + (kq >> 1)) * 8 + 2 * q + (kq & 1)];
    }
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) f.a2[m][r][m2] = W2[(16 * m2 + row) * 32 + 16 * m + 4 * kq + r];
#pragma unroll
        for (int r = 0; r < 4; ++r) f.bias[m2][r] = b2[16 * m2 + 4 * kq + r];
    }
}

// v_cmp_class_f32 mask: signalling NaN | quiet NaN | -inf | +inf
constexpr int kClassNonFinite = 0x1 | 0x2 | 0x4 | 0x200;

__device__ __forceinline__ bool non_finite(float x) { return __builtin_amdgcn_classf(x, kClassNonFinite); }

// ---- source volume -> LDS (channel-last, padded) ---------------------------------
// Returns whether this thread met a NaN / inf voxel (the project's rule for non-finite inputs, ahv_exact.h); a caller
// that does not ask uses stage_src_volume, where the test folds away.
__device__ __forceinline__ bool stage_src_volume_scan(float* srcT, const float* __restrict__ vol, int tid, int nthreads)
{
    bool bad = false;
    for (int i = tid; i < 16 * 512; i += nthreads) {
        const int c = i >> 9, v = i & 511;
        const float x = vol[i];
        bad = bad || non_finite(x);
        srcT[((v >> 6) * kSrcPlaneRows + ((v >> 3) & 7) * kSrcRowsY + (v & 7)) * kSrcStride + c] = x;
    }
    return bad;
}

__device__ __forceinline__ void stage_src_volume(float* srcT, const float* __restrict__ vol, int tid,
                                                 int nthreads)
{
    (void)stage_src_volume_scan(srcT, vol, tid, nthreads);
}

// ---- GEMM1 on one quarter ---------------------------------------------------------
// u[o][i][j] += sum_{c,k} W1x[o][c,k] V'[c][i][j][k] + W1y[o][c,k] V'[c][i][k][j] + W1z[o][c,k] V'[c][k][i][j]
// (modules/modules.py:115-120) restricted to the voxels d in {2Q,2Q+1} of V':
//   x slab: positions (d,h) of this quarter = n-tile Q, all k=(c,w)      -> 64 MFMA
//   y slab: positions (d,w) of this quarter = n-tile Q, all k=(c,h)      -> 64 MFMA
//   z slab: all positions (h,w) = 4 n-tiles,  k=(c,d) for the 2 d's      -> 64 MFMA
template <int Q>
__device__ __forceinline__ void gemm1_quarter(f32x4 (&acc)[2][4], const HeadFrags& f, const float* buf,
                                              int lane)
{
    const int n = lane & 15, kq = lane >> 4;
    const int i0 = n >> 3, j = n & 7;
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int eh = 0; eh < 2; ++eh) {
            const float bx = buf[c * 128 + qoff(i0, j, 4 * eh + kq)];
            acc[0][Q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.ax[c][eh][0], bx, acc[0][Q], 0, 0, 0);
            acc[1][Q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.ax[c][eh][1], bx, acc[1][Q], 0, 0, 0);
        }
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int bh = 0; bh < 2; ++bh) {
            const float by = buf[c * 128 + qoff(i0, 4 * bh + kq, j)];
            acc[0][Q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.ay[c][bh][0], by, acc[0][Q], 0, 0, 0);
            acc[1][Q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.ay[c][bh][1], by, acc[1][Q], 0, 0, 0);
        }
#pragma unroll
    for (int cp = 0; cp < 8; ++cp)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float bz = buf[(2 * cp + (kq >> 1)) * 128 + qoff(kq & 1, 2 * t + i0, j)];
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.az[Q][cp][0], bz, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.az[Q][cp][1], bz, acc[1][t], 0, 0, 0);
        }
}

// ---- ReLU + GEMM2 + bias straight from the accumulators ----------------------------
// v = W2 relu(u) + b2 (modules/modules.py:68-69).  Register r of accumulator tile (m,t)
// holds u[16m + 4kq + r][pos]: exactly the B operand of a k-step whose four k values are
// {16m + 4kq + r}, so no lane movement and no LDS round trip is needed.
__device__ __forceinline__ void gemm2(f32x4 (&v)[2][4], const f32x4 (&acc)[2][4], const HeadFrags& f)
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        v[0][t] = f.bias[0];
        v[1][t] = f.bias[1];
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float a = acc[m][t][r];
                const float u = a < 0.0f ? 0.0f : a;  // F.relu: a NaN stays a NaN (v_max would drop it)
                v[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[m][r][0], u, v[0][t], 0, 0, 0);
                v[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a2[m][r][1], u, v[1][t], 0, 0, 0);
            }
}

// ---- packed (score, index) keys ---------------------------------------------------
// key = ordered_i32(score) << 32 | (0xFFFFFFFF - idx) as a SIGNED 64-bit integer: signed max = largest score,
// lowest index among equals (torch.max, test_co3d.py:145).  NaN orders above +inf.  Signed order so that the key is
// what an int64 MAX all-reduce (RCCL, gloo, torch.max) wants as it is -- no re-biasing launch on either side of the
// collective.  kKeyEmpty (INT64_MIN) is below every real key: "nothing scored yet".
typedef long long key_t;
constexpr key_t kKeyEmpty = (key_t)0x8000000000000000ull;

__device__ __forceinline__ key_t pack_key(float s, unsigned idx)
{
    s += 0.0f;  // -0 -> +0 so that equal values compare equal
    unsigned u = __float_as_uint(s);
    if (s != s) u = 0x7FC00000u;  // canonical quiet NaN: ranks highest
    u = (u & 0x80000000u) ? (u ^ 0x7FFFFFFFu) : u;  // negative floats: larger magnitude = smaller integer
    return (key_t)(((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx));
}

__device__ __forceinline__ float key_score(key_t key)
{
    unsigned u = (unsigned)((unsigned long long)key >> 32);
    u = (u & 0x80000000u) ? (u ^ 0x7FFFFFFFu) : u;
    return __uint_as_float(u);
}

__device__ __forceinline__ long key_index(key_t key) { return (long)(0xFFFFFFFFu - (unsigned)((unsigned long long)key & 0xFFFFFFFFull)); }

}  // namespace ahv

#include "ahv_wave.h"  // the wave reductions (wave_max_key, wave_max_key_dpp, wave_sum_dpp, ...): they need key_t
