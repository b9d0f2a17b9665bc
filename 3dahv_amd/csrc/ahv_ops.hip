// ahv_ops.hip -- op-level drop-in kernels: each materialises the tensor the
// reference's corresponding call returns, so the reference's own call sequence
// (rotate_volume -> forward_3d2d -> mul/sum/mean -> max) runs unchanged on HIP.
// These are the HBM-bound siblings of the fused scorer (ahv_score.hip): forward_3d2d* and score_features here, rotate_volume
// and its adjoint in ahv_rotate.hip.  Also here: the hypothesis generators (random_rotations, so3_grid) and the library's
// zero fill.  What happens once the scores exist -- the arg-max of that sequence, lists, modes, ascent -- is ahv_select.hip,
// with the multi-view kernels in ahv_views.hip and the posterior and its draws in ahv_posterior.hip; tracking a pose over a
// frame sequence is ahv_track.hip.
#include "ahv_device.h"
#include "ahv_launch.h"
#include "ahv_dual.h"
#include "ahv_exact.h"
#include "ahv_so3.h"

namespace ahv {

// ---------------------------------------------------------------------------------
// forward_3d2d (modules/modules.py:112-124) on materialised volumes [M][16][8][8][8].
// Same wave-per-item MFMA contraction as the fused scorer; the quarter buffers are
// filled from HBM instead of by the trilinear gather.  32 KiB in + 8 KiB out per item.
// ---------------------------------------------------------------------------------
constexpr int kF32Threads = 256;
constexpr int kF32LdsFloats = 4 * 2 * kQuarterFloats;

// F.normalize's denominator, |v|.clamp_min(eps): torch's clamp KEEPS a NaN norm (a column that holds +-inf beside NaN is NaN
// throughout), where fmaxf hands back eps and leaves the +-inf in the column.  For every norm that is a number, fmaxf's value.
__device__ __forceinline__ float clamped_norm(float ss)
{
    const float nrm = sqrtf(ss);
    return nrm < 1e-12f ? 1e-12f : nrm;
}

// A lane's share of |v|^2: its 2 x 4 channels of one position.  The association is spelled out -- element 1's square rounded
// on its own, element 0 joined to it by FMA, then 2, 3 and the second four in order -- because it is what the compiler made of
// `ss += v * v` while an fmaxf stood behind the loop; with the select of clamped_norm there it left the same loop as separate
// multiplies and adds, and the features' last bits moved.
__device__ __forceinline__ float sumsq8(const f32x4& a, const f32x4& b)
{
    float ss = a[1] * a[1];
    ss = fmaf(a[0], a[0], ss);
    ss = fmaf(a[2], a[2], ss);
    ss = fmaf(a[3], a[3], ss);
#pragma unroll
    for (int r = 0; r < 4; ++r) ss = fmaf(b[r], b[r], ss);
    return ss;
}

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
            float ss = sumsq8(v[0][t], v[1][t]);
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            const float nrm = clamped_norm(ss);
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
            float ss = sumsq8(v[0][t], v[1][t]);
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            // v / max(|v|, eps) as v * (1 / max(|v|, eps)): ONE correctly rounded division per position instead of eight per
            // lane (an IEEE division is ~10 vector instructions, and fp32 MFMAs overlap none of them: 320 of an item's ~900);
            // each feature within 1 ulp of the quotient
            const float inv = 1.0f / clamped_norm(ss);
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
    if ((reinterpret_cast<unsigned long long>(W1) & 15ull) == 0) {
        for (int i = tid; i < 32 * 96; i += 512) {  // 96 float4 per W1 row
            const int r = i / 96, k4 = i - r * 96;
            const f32x4 w = *reinterpret_cast<const f32x4*>(W1 + r * 384 + 4 * k4);
            float* d = w1s + r * kW1PadStride + 4 * k4;
            d[0] = w[0]; d[1] = w[1]; d[2] = w[2]; d[3] = w[3];
        }
    } else {  // a view that starts off a 16-byte boundary (stage_w1_table's rule): same map, one float at a time
        for (int i = tid; i < 32 * 384; i += 512) w1s[(i / 384) * kW1PadStride + i % 384] = W1[i];
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
    float ss = sumsq8(v[0], v[1]);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    const float nrm = clamped_norm(ss);
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
// reproducibly, and the call is graph-capturable.  The sampler is haar_rotation (ahv_so3.h).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void random_rotations_kernel(unsigned long long seed, unsigned long long offset, long N,
                                                               float* __restrict__ out)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    haar_rotation(seed, offset + (unsigned long long)n, out + n * 9);
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

// Rows with the caller's bytes between them (ahv_rotate_volume_backward_f32 with a padded batch stride): one float per
// thread, row by row over gridDim.y, nothing between the rows is touched.
__global__ __launch_bounds__(256) void zero_fill_strided_kernel(float* __restrict__ p, long elems, long stride, long rows)
{
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    for (long r = blockIdx.y; r < rows; r += gridDim.y)
        for (long i = i0; i < elems; i += step) p[r * stride + i] = 0.0f;
}

hipError_t launch_zero_fill_strided(float* p, int64_t elems, int64_t stride, int64_t rows, hipStream_t stream)
{
    if (elems <= 0 || rows <= 0) return hipSuccess;
    if (stride < elems) return hipErrorInvalidValue;
    const int64_t bx = (elems + 255) / 256;
    hipLaunchKernelGGL(zero_fill_strided_kernel, dim3((unsigned)(bx < 64 ? bx : 64), (unsigned)(rows < 1024 ? rows : 1024)),
                       dim3(256), 0, stream, p, (long)elems, (long)stride, (long)rows);
    return hipGetLastError();
}

}  // namespace ahv
