// ahv_enc_rows.h -- the attention and row kernels of the encoder, included by ahv_encoder.hip behind ahv_enc_linear.h
// (f32x4, glds16):
//
//   attention_heads_kernel        softmax(Q K^T / 8) V and the output projection, four waves per (sample, head, 16 queries)
//   attention_sample_head_kernel  the same with one workgroup per (sample, head), for many samples
//   ln_kernel                     LayerNorm(sum_ks P + bias) fused with cat([x, .]) or x + .   (attention.py:255-258)
//   nchw_to_tokens_kernel, groupnorm_kernel, finish_kernel   around the token stage (forward_2d3d)
#pragma once
#include "ahv_enc_linear.h"

namespace ahv {

__device__ __forceinline__ float wave_sum(float x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// -------------------------------------------------------------------------------------------------
// Attention + output projection in one launch (CrossAttention.forward, transformer/attention.py:214-237, up to but
// not including to_out's bias).
// -------------------------------------------------------------------------------------------------
struct AttnOutProb {
    const float *Q, *K, *V;
    const float* Wo;  // [256][256] to_out.0.weight
    float* P;         // [M][256]
    long ldq, ldkv;
};
struct AttnOutArgs {
    AttnOutProb p[2];
    int B;
    float scale;
#ifdef AHV_ENC_PROBE
    unsigned long long* stamps;
#endif
};

// -------------------------------------------------------------------------------------------------
// The four waves of a workgroup cooperate on ONE head of one 16-query tile: grid = (B * nprob, 4 query tiles,
// 4 heads).  (Round 2's first form gave every wave a whole head and repeated the attention per column quarter: 192
// dependent MFMAs per wave, 9.2 us at B = 1; this one 6.5 us.)  Wave w scores key tile w
// (16 MFMAs), the four partial softmaxes are merged through 128 bytes of LDS with the online-softmax identity
// (p_w = exp(s - m_w); m = max m_w; L = sum l_w exp(m_w - m); P = p_w exp(m_w - m) / L: ONE barrier), wave w forms its
// keys' share of O^T (16 MFMAs), the shares meet in LDS, and wave w then contracts the head's O with column quarter
// w of W_out (64 MFMAs).  96 dependent MFMAs per wave instead of 192, a quarter of the K / V loads.  The result is
// one split-K slab PER HEAD, P[h][M][256]; ln_kernel sums the four.
// -------------------------------------------------------------------------------------------------
// One query tile per workgroup.  Walking 2 or 4 tiles of a (sample, head) with the K, V and W_out fragments held in registers
// (round 6) changed nothing at B = 32 -- 1 964 / 1 958 / 1 960 us per forward for 1 / 2 / 4 tiles, 17.6-18.1 us per launch
// either way: the launch is bound by the dependent chain of a tile (16 + 16 + 64 MFMAs, two barriers, a softmax), not by its
// 100 MB of L2 reads (HISTORY.md; the multi-tile code was last in commit 86a1f1c).
__global__ __launch_bounds__(256) void attention_heads_kernel(const AttnOutArgs a, int M)
{
    __shared__ float sm[4][16][2];                                   // per wave and query: (max, sum)
    __shared__ __attribute__((aligned(16))) float so[4][4][64][4];   // per wave: O^T share [dt][lane][r]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pi = (int)blockIdx.x / a.B, b = (int)blockIdx.x - pi * a.B;
    const AttnOutProb pr = a.p[pi];
    const int it = blockIdx.y, h = blockIdx.z;
    const int c16 = lane & 15, kq = lane >> 4;
    const float* q = pr.Q + (long)(b * 64 + it * 16 + c16) * pr.ldq + h * 64 + 4 * kq;
    const float* k = pr.K + (long)(b * 64 + w * 16 + c16) * pr.ldkv + h * 64 + 4 * kq;
    const float* v = pr.V + (long)(b * 64 + w * 16 + 4 * kq) * pr.ldkv + h * 64 + c16;
    AHV_ENC_STAMP(0);
    // every operand is requested before the first MFMA
    f32x4 ka[4], qb[4], wf[4][4];
    float va[4][4];  // [r][dt]: V[16 w + 4 kq + r][16 dt + c16]
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
        qb[ds] = *reinterpret_cast<const f32x4*>(q + 16 * ds);
        ka[ds] = *reinterpret_cast<const f32x4*>(k + 16 * ds);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) va[r][dt] = v[(long)r * pr.ldkv + dt * 16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            wf[nt][dt] = *reinterpret_cast<const f32x4*>(pr.Wo + (long)(w * 64 + nt * 16 + c16) * 256 + h * 64 + 16 * dt + 4 * kq);
    __builtin_amdgcn_sched_barrier(0);
    // One trip: what remains of the multi-tile form.  hipcc schedules the loads above and the chain below as separate
    // regions because of the loop; without it, it emits a different (unmeasured) schedule.
#pragma unroll 1
    for (int t = 0; t < 1; ++t) {
        // S^T[j = 16 w + 4 kq + r][i = c16]
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < 4; ++ds)
#pragma unroll
            for (int s = 0; s < 4; ++s) st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[ds][s], qb[ds][s], st, 0, 0, 0);
        AHV_ENC_STAMP(1);
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            st[r] *= a.scale;
            m = fmaxf(m, st[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            st[r] = expf(st[r] - m);
            l += st[r];
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if (kq == 0) {
            sm[w][c16][0] = m;
            sm[w][c16][1] = l;
        }
        AHV_ENC_STAMP(2);
        __syncthreads();
        AHV_ENC_STAMP(3);
        float mg = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) mg = fmaxf(mg, sm[u][c16][0]);
        float L = 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) L += sm[u][c16][1] * expf(sm[u][c16][0] - mg);
        const float f = expf(m - mg) / L;
        // this wave's share of O^T[d = 16 dt + 4 kq + r][i = c16]
        f32x4 ot[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = st[r] * f;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) ot[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[r][dt], p, ot[dt], 0, 0, 0);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(&so[w][dt][lane][0]) = ot[dt];
        AHV_ENC_STAMP(4);
        __syncthreads();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            ot[dt] = *reinterpret_cast<const f32x4*>(&so[0][dt][lane][0]);
#pragma unroll
            for (int u = 1; u < 4; ++u) ot[dt] += *reinterpret_cast<const f32x4*>(&so[u][dt][lane][0]);
        }
        // column quarter w of the head's output projection: D^T[n = 64 w + 16 nt + 4 kq + r][q = c16]
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nt][dt][r], ot[dt][r], acc[nt], 0, 0, 0);
        float* out = pr.P + ((long)h * M + b * 64 + it * 16 + c16) * 256 + w * 64 + 4 * kq;
        asm volatile("" :: "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]));
        AHV_ENC_STAMP(5);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<f32x4*>(out + nt * 16) = acc[nt];
        AHV_ENC_STAMP(6);
    }
}

// -------------------------------------------------------------------------------------------------
// The same launch for MANY samples (B >= 24, round 6): one workgroup per (sample, head), wave w owns the 16 queries of
// tile w against ALL 64 keys.  The in-kernel timeline of the kernel above at B = 32 (tools/kbench_enc.bin 32 --stamps,
// profiles/r06_attention_timeline_b32.txt) showed what its 17.9 us are: 1 024 workgroups of ~150 registers run three per CU,
// so a quarter of them waits 11 us for a slot; every workgroup spends its first 4.2 us fetching 100 KB of operands with
// fragment-shaped loads (64 KB of them W_out: 64 MB over the grid for a 256 KB matrix) and then 6.3 us in a chain of 96
// MFMAs, two barriers and a softmax whose every vector instruction queues behind the other waves' MFMAs.  Here a wave has
// whole softmax rows (no merge, no barrier between scores and P V), four independent MFMA chains in every phase (64 + 64 +
// 256 MFMAs per wave), every operand arrives ONCE per workgroup as full 256-byte rows by LDS-DMA, and W_out's head slice
// travels while softmax and P V run: 256 workgroups at B = 32, one per CU, 29 MB of operand traffic.
// Same math as above (softmax over the 64 keys in one pass: p = exp2((s - max) scale log2 e) / sum), same output: one
// split-K slab per head.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_sample_head_kernel(const AttnOutArgs a, int M)
{
    // ONE LDS object (see linear_tile_kernel): row-major images [row][64 d] of the head's Q, K, V (64 rows each) and W_out
    // slice (256 rows), 16-byte chunks XOR-swizzled per row on the SOURCE side (the images are filled by LDS-DMA: lane-linear)
    constexpr int kQ = 0, kK = 64 * 64, kV = 2 * 64 * 64, kW = 3 * 64 * 64;
    __shared__ __attribute__((aligned(1024))) float img[kW + 256 * 64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pi = (int)blockIdx.x / a.B, b = (int)blockIdx.x - pi * a.B;
    const AttnOutProb pr = a.p[pi];
    const int h = blockIdx.y;
    const int c16 = lane & 15, kq = lane >> 4;
    AHV_ENC_STAMP(0);
    // Every operand comes through LDS in 1 KiB pieces of four 256-byte rows (lane -> row lane / 16, chunk lane % 16): the
    // fragment-shaped loads of the kernel above put 16 lanes on 16 different rows (16 quads x 4 segments = 64 cycles of the
    // CU's address unit per instruction; with 36 of them per wave the first 3.5 us of the workgroup), these take 16.
    // Chunk swizzles (conflict-free for the ds_read_b128 lane groups, checked in DESIGN 4.3): Q, K: c ^ (row % 16);
    // V: c ^ (row % 4); W_out: c ^ rot(row % 16), rot = the nibble's two bit pairs exchanged.
    const int prow = lane >> 4, pch = lane & 15;
    {
        const long r0 = b * 64 + 16 * w;   // wave w fetches rows 16 w .. 16 w + 15 of Q, K and V
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * i + prow;   // row % 16
            glds16(pr.Q + (r0 + row) * pr.ldq + h * 64 + 4 * (pch ^ row), img + kQ + (16 * w + 4 * i) * 64 + 4 * lane);
            glds16(pr.K + (r0 + row) * pr.ldkv + h * 64 + 4 * (pch ^ row), img + kK + (16 * w + 4 * i) * 64 + 4 * lane);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * i + prow;
            glds16(pr.V + (r0 + row) * pr.ldkv + h * 64 + 4 * (pch ^ (row & 3)), img + kV + (16 * w + 4 * i) * 64 + 4 * lane);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0)
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    f32x4 qb[4], ka[4][4], va[4][4];   // va[j][r][dt] = V[key 16 j + 4 kq + r][d = 4 c16 + dt]
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
        qb[ds] = *reinterpret_cast<const f32x4*>(img + kQ + (16 * w + c16) * 64 + 4 * ((4 * ds + kq) ^ c16));
#pragma unroll
        for (int j = 0; j < 4; ++j) ka[j][ds] = *reinterpret_cast<const f32x4*>(img + kK + (16 * j + c16) * 64 + 4 * ((4 * ds + kq) ^ c16));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) va[j][r] = *reinterpret_cast<const f32x4*>(img + kV + (16 * j + 4 * kq + r) * 64 + 4 * (c16 ^ r));
    // The head dimension is walked in two orders: d = 16 ds + 4 kq + s for Q K^T (a lane's four consecutive d are MFMA
    // k-steps) and d = 16 kq + 4 r + dt for P V and the projection (a lane's four consecutive d are the four d-TILES: tile
    // dt = {d : d mod 4 = dt}) -- any order serves a contraction as long as both operands use it.
    // S^T[key = 16 j + 4 kq + r][query = c16], four independent chains
    f32x4 st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < 4; ++ds)
#pragma unroll
        for (int sx = 0; sx < 4; ++sx)
#pragma unroll
            for (int j = 0; j < 4; ++j) st[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[j][ds][sx], qb[ds][sx], st[j], 0, 0, 0);
    // W_out rows 64 w .. 64 w + 63 of the head's slice (16 pieces).  Requested HERE, with every fragment of Q, K and V in
    // registers: hipcc drains LDS-DMA in front of any ds_read of the same object, so nothing is read between this point and
    // the barrier in front of the projection -- the pieces travel while softmax and P V run.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(va[j][r]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = 64 * w + 4 * i + prow, r16 = row & 15;
        glds16(pr.Wo + (long)row * 256 + h * 64 + 4 * (pch ^ (((r16 & 3) << 2) | (r16 >> 2))), img + kW + (64 * w + 4 * i) * 64 + 4 * lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    AHV_ENC_STAMP(1);
    const float c = a.scale * 1.44269504088896341f;
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            st[j][r] *= c;
            m = fmaxf(m, st[j][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            st[j][r] = __builtin_amdgcn_exp2f(st[j][r] - m);
            l += st[j][r];
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    AHV_ENC_STAMP(2);
    // O^T[d = 4 (4 kq + r) + dt][query = c16] in tile dt
    f32x4 ot[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = st[j][r] * inv;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) ot[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[j][r][dt], p, ot[dt], 0, 0, 0);
        }
    AHV_ENC_STAMP(3);
    __builtin_amdgcn_sched_barrier(0);    // (MFMAs on registers would otherwise be free to move across the barrier)
    __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0): this wave's W_out pieces are in LDS
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    AHV_ENC_STAMP(4);
    // the head's output projection for this wave's 16 queries: D^T[n = 16 nt + 4 kq + r][query = c16], four n-tiles at a time;
    // k-step (dt, r) contracts d = 16 kq + 4 r + dt: B = ot[dt][r], A = component dt of W_out[16 nt + c16][16 kq + 4 r ..]
    float* out = pr.P + ((long)h * M + b * 64 + 16 * w + c16) * 256 + 4 * kq;
    const float* wrow = img + kW + c16 * 64;
    const int wsw = ((c16 & 3) << 2) | (c16 >> 2);
#pragma unroll
    for (int ng = 0; ng < 4; ++ng) {
        f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x4 wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const f32x4*>(wrow + 16 * (4 * ng + i) * 64 + 4 * ((4 * kq + r) ^ wsw));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][dt], ot[dt][r], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(out + 16 * (4 * ng + i)) = acc[i];
    }
    AHV_ENC_STAMP(6);
}

// -------------------------------------------------------------------------------------------------
// Row kernels (one wave per 256-wide row; blockIdx.y = problem).
// -------------------------------------------------------------------------------------------------
struct LnProb {
    const float* P;     // [KS][M][256] split-K slabs of the preceding linear
    const float* bias;  // [256]
    const float* g;     // LayerNorm weight
    const float* be;    // LayerNorm bias
    const float* x;     // [M][256] block input (copied into cat / added as residual)
    float* out;         // CONCAT: cat [M][512];  else: block output [M][256]
};
struct LnArgs {
    LnProb p[2];
    int KS, M;
};

// LayerNorm(256, eps 1e-5, biased variance) of (sum_ks P + bias);
// CONCAT: out[row] = [x[row], y]   (attention.py:255-256)   else: out[row] = x[row] + y   (:257-258)
// KS is a template parameter so that the slab loads are independent instructions issued together: with a run-time
// trip count hipcc keeps the loop rolled and every slab costs its own memory round trip.
template <bool CONCAT, int KS>
__global__ __launch_bounds__(256) void ln_kernel(const LnArgs a)
{
    const LnProb pr = a.p[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.M) return;
    f32x4 slab[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) slab[ks] = *reinterpret_cast<const f32x4*>(pr.P + ((long)ks * a.M + row) * 256 + 4 * lane);
    const f32x4 xin = *reinterpret_cast<const f32x4*>(pr.x + (long)row * 256 + 4 * lane);
    const f32x4 gam = *reinterpret_cast<const f32x4*>(pr.g + 4 * lane), bet = *reinterpret_cast<const f32x4*>(pr.be + 4 * lane);
    f32x4 t = *reinterpret_cast<const f32x4*>(pr.bias + 4 * lane);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) t += slab[ks];
    const float mean = wave_sum(t[0] + t[1] + t[2] + t[3]) * (1.0f / 256.0f);
    const f32x4 d = t - mean;
    const float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 256.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    const f32x4 y = d * rstd * gam + bet;
    if (CONCAT) {
        *reinterpret_cast<f32x4*>(pr.out + (long)row * 512 + 4 * lane) = xin;
        *reinterpret_cast<f32x4*>(pr.out + (long)row * 512 + 256 + 4 * lane) = y;
    } else {
        *reinterpret_cast<f32x4*>(pr.out + (long)row * 256 + 4 * lane) = xin + y;
    }
}

// -------------------------------------------------------------------------------------------------
// Kernels around the token stage (Feature_Aligner.forward_2d3d, modules/modules.py:86-101).
// Activations live token-major [M = 64*B][C] ("channel-last"); blockIdx.y = stream.
// -------------------------------------------------------------------------------------------------
struct Nchw2TokArgs {
    const float* in[2];  // [B][C][64]
    float* out[2];       // [B*64][C]
    int C, B;
    float* zero;         // 16 floats the first workgroup clears: the zero row of the implicit-GEMM convolutions
};

__global__ __launch_bounds__(256) void nchw_to_tokens_kernel(const Nchw2TokArgs a)
{
    __shared__ float tile[64][65];
    const float* in = a.in[blockIdx.z];
    float* out = a.out[blockIdx.z];
    const int b = blockIdx.y, c0 = blockIdx.x * 64;
    if (a.zero != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < 16) a.zero[threadIdx.x] = 0.0f;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, m = i & 63;
        tile[c][m] = in[((long)b * a.C + c0 + c) * 64 + m];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int m = i >> 6, c = i & 63;
        out[((long)b * 64 + m) * a.C + c0 + c] = tile[c][m];
    }
}

// GroupNorm(32 groups, eps 1e-6, biased variance) over (8 channels x 64 tokens) of one sample
// (transformer/attention.py:120-121,378,383): one wave per (sample, group), lane = token.
struct GnArgs {
    const float* x[2];
    float* y[2];
    const float *g, *be;
    int B;
};

__global__ __launch_bounds__(256) void groupnorm_kernel(const GnArgs a)
{
    const int lane = threadIdx.x & 63;
    const int grp = blockIdx.x * 4 + (threadIdx.x >> 6);  // 0..31
    const int b = blockIdx.y;
    const float* x = a.x[blockIdx.z] + ((long)b * 64 + lane) * 256 + grp * 8;
    float* y = a.y[blockIdx.z] + ((long)b * 64 + lane) * 256 + grp * 8;
    const f32x4 u = *reinterpret_cast<const f32x4*>(x), v = *reinterpret_cast<const f32x4*>(x + 4);
    const float mean = wave_sum(u[0] + u[1] + u[2] + u[3] + v[0] + v[1] + v[2] + v[3]) * (1.0f / 512.0f);
    const f32x4 du = u - mean, dv = v - mean;
    const float var = wave_sum(du[0] * du[0] + du[1] * du[1] + du[2] * du[2] + du[3] * du[3] + dv[0] * dv[0] +
                               dv[1] * dv[1] + dv[2] * dv[2] + dv[3] * dv[3]) * (1.0f / 512.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-6f);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.g + grp * 8), g1 = *reinterpret_cast<const f32x4*>(a.g + grp * 8 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.be + grp * 8), b1 = *reinterpret_cast<const f32x4*>(a.be + grp * 8 + 4);
    *reinterpret_cast<f32x4*>(y) = du * rstd * g0 + b0;
    *reinterpret_cast<f32x4*>(y + 4) = dv * rstd * g1 + b1;
}

// Generic finish: v = sum_ks P[ks][m][n] (+ bias[n]); relu on columns < relu_cols; + res[m][n]; + pe[m % 64][n];
// stored as  layout 0: out[m][ldo] token-major
//            layout 1: channel-last volume from tokens, out[b][d][h][w][c'] with token m = (b, h*8+w), n = c'*8 + d
//                      (the reshape(bs, 32, 8, 8, 8) of modules/modules.py:97)
//            layout 2: NCDHW, out[b][n][voxel] with row m = (b, voxel)            (the scorer's volume layout)
//            layout 3: columns [0, N/2) to out[m][N/2], columns [N/2, N) to out2[m][N/2]   (the 3-D res-block's first
//                      conv carries its 1x1x1 skip as extra output columns: one pass splits them)
struct FinProb {
    const float* P;
    const float* bias;
    const float* res;
    float* out;
    float* out2;
};
struct FinArgs {
    FinProb p[2];
    const float* pe;
    int KS, M, N, ldp, col0;  // P slabs are [KS][M][ldp]; columns col0 .. col0+N-1 are used
    int relu_cols, ldres, ldo, layout;
};

template <int KS>  // compile-time: every slab (and the optional operands) is requested before the first add
__global__ __launch_bounds__(256) void finish_kernel(const FinArgs a)
{
    const FinProb pr = a.p[blockIdx.y];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int n4 = a.N >> 2;
    if (i >= (long)a.M * n4) return;
    const int m = (int)(i / n4), n = (int)(i - (long)m * n4) * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 slab[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) slab[ks] = *reinterpret_cast<const f32x4*>(pr.P + ((long)ks * a.M + m) * a.ldp + a.col0 + n);
    const f32x4 res = pr.res ? *reinterpret_cast<const f32x4*>(pr.res + (long)m * a.ldres + n) : zero;
    const f32x4 pe = a.pe ? *reinterpret_cast<const f32x4*>(a.pe + (long)(m & 63) * a.N + n) : zero;
    f32x4 v = pr.bias ? *reinterpret_cast<const f32x4*>(pr.bias + n) : zero;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) v += slab[ks];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (n + e < a.relu_cols) v[e] = fmaxf(v[e], 0.0f);
    v += res;
    v += pe;
    if (a.layout == 0) {
        *reinterpret_cast<f32x4*>(pr.out + (long)m * a.ldo + n) = v;
    } else if (a.layout == 1) {
        const int b = m >> 6, hw = m & 63, cp = n >> 3, d0 = n & 7;
#pragma unroll
        for (int e = 0; e < 4; ++e) pr.out[(((long)b * 8 + d0 + e) * 64 + hw) * 32 + cp] = v[e];
    } else if (a.layout == 3) {
        const int h = a.N >> 1;
        float* dst = n < h ? pr.out + (long)m * h + n : pr.out2 + (long)m * h + (n - h);
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        const int b = m >> 9, vox = m & 511;
#pragma unroll
        for (int e = 0; e < 4; ++e) pr.out[((long)b * a.N + n + e) * 512 + vox] = v[e];
    }
}

}  // namespace ahv
