// ahv_so3.h -- the counter-based rotation sampler shared by the hypothesis generators (ahv_ops.hip) and the tracker's predict
// step (ahv_track.hip): Philox-4x32-10 -> 4 uniforms -> Box-Muller -> normalised Gaussian quaternion -> matrix.
#pragma once
#include "ahv_device.h"

namespace ahv {

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// (qr, qi, qj, qk) of any norm > 0 -> the nine matrix entries at o
__device__ __forceinline__ void quaternion_matrix(float qr, float qi, float qj, float qk, float* __restrict__ o)
{
    const float t = 2.0f / fmaxf(qr * qr + qi * qi + qj * qj + qk * qk, 1e-30f);
    o[0] = 1.0f - t * (qj * qj + qk * qk); o[1] = t * (qi * qj - qk * qr);        o[2] = t * (qi * qk + qj * qr);
    o[3] = t * (qi * qj + qk * qr);        o[4] = 1.0f - t * (qi * qi + qk * qk); o[5] = t * (qj * qk - qi * qr);
    o[6] = t * (qi * qk - qj * qr);        o[7] = t * (qj * qk + qi * qr);        o[8] = 1.0f - t * (qi * qi + qj * qj);
}

// Four uniforms of one Philox block -> two Box-Muller pairs (g0, g1), (g2, g3): standard normal, independent.
__device__ __forceinline__ void box_muller4(const unsigned (&c)[4], float& g0, float& g1, float& g2, float& g3)
{
    // uniforms in (0,1]: never log(0)
    const float u0 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2] >> 8) + 1.0f) * (1.0f / 16777216.0f), u3 = (float)(c[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u1, &s0, &c0);
    sincosf(6.28318530717958647692f * u3, &s1, &c1);
    g0 = r0 * c0; g1 = r0 * s0; g2 = r1 * c1; g3 = r1 * s1;
}

// Rotation `ctr` of the Haar stream of `seed`: what ahv_random_rotations_f32 writes for offset + n = ctr, bit for bit
// (random_rotations_kernel and the fresh slots of the predict kernels all call it).  Not inlined: a call keeps the callers'
// register counts where DESIGN 4.2 records them; `inline` because the definition sits in a header.
__device__ __noinline__ inline void haar_rotation(unsigned long long seed, unsigned long long ctr, float* __restrict__ o)
{
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0x3D4148u, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    float qr, qi, qj, qk;
    box_muller4(c, qr, qi, qj, qk);
    quaternion_matrix(qr, qi, qj, qk, o);
}

}  // namespace ahv
