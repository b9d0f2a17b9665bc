// ahv_so3.h -- the counter-based rotation sampler shared by the hypothesis generators (ahv_ops.hip) and the tracker's predict
// step (ahv_track.hip): Philox-4x32-10 -> 4 uniforms -> Box-Muller -> normalised Gaussian quaternion -> matrix.  Below it the two
// compositions more than one source needs bit for bit: R exp([w]x) as unit quaternions (ahv_track.hip, ahv_graph.hip) and Q A^T
// with the bits of view_rotations_kernel (ahv_views.hip, ahv_graph.hip).
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

// o = M(normalise(q(r) q(w))), the matrix of r exp([w]x), composed as unit quaternions and normalised.
__device__ __forceinline__ void compose_rotation_vector(const float (&r)[9], float w0, float w1, float w2, float* __restrict__ o)
{
    const float a = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
    // q(w) = (cos a/2, sin(a/2) w / a); sin(a/2) / a -> 1/2 - a^2/48 as a -> 0
    float sh, ch;
    sincosf(0.5f * a, &sh, &ch);
    const float kq = a < 1e-3f ? 0.5f - a * a * (1.0f / 48.0f) : sh / a;
    const float dr = ch, di = kq * w0, dj = kq * w1, dk = kq * w2;
    // q(R) by Shepperd's branch: divide by the largest of the four components
    float qr, qi, qj, qk;
    const float tr = r[0] + r[4] + r[8];
    if (tr > 0.0f) {
        const float s = 2.0f * sqrtf(tr + 1.0f);
        qr = 0.25f * s; qi = (r[7] - r[5]) / s; qj = (r[2] - r[6]) / s; qk = (r[3] - r[1]) / s;
    } else if (r[0] > r[4] && r[0] > r[8]) {
        const float s = 2.0f * sqrtf(1.0f + r[0] - r[4] - r[8]);
        qr = (r[7] - r[5]) / s; qi = 0.25f * s; qj = (r[1] + r[3]) / s; qk = (r[2] + r[6]) / s;
    } else if (r[4] > r[8]) {
        const float s = 2.0f * sqrtf(1.0f + r[4] - r[0] - r[8]);
        qr = (r[2] - r[6]) / s; qi = (r[1] + r[3]) / s; qj = 0.25f * s; qk = (r[5] + r[7]) / s;
    } else {
        const float s = 2.0f * sqrtf(1.0f + r[8] - r[0] - r[4]);
        qr = (r[3] - r[1]) / s; qi = (r[2] + r[6]) / s; qj = (r[5] + r[7]) / s; qk = 0.25f * s;
    }
    // Hamilton product q(R) q(w): the matrix of a product is the product of the matrices, R exp([w]x)
    float pr = qr * dr - qi * di - qj * dj - qk * dk;
    float pi = qr * di + qi * dr + qj * dk - qk * dj;
    float pj = qr * dj - qi * dk + qj * dr + qk * di;
    float pk = qr * dk + qi * dj - qj * di + qk * dr;
    const float inv = 1.0f / sqrtf(fmaxf(pr * pr + pi * pi + pj * pj + pk * pk, 1e-30f));
    pr *= inv; pi *= inv; pj *= inv; pk *= inv;
    quaternion_matrix(pr, pi, pj, pk, o);
}

// o = Q_n A_v^T with the bits of view_rotations_kernel (q = Q_n, d = A_v: entry (a, c) is row a of Q_n times row c of A_v).
// That kernel states the entry as p0 + p1 + p2 and leaves the contraction to the compiler, which -- vectorising the nine entries
// in pairs -- does not contract them alike: the last product is always fused, fma(q2, d2, .), onto fma(q0, d0, rn(p1)) in
// columns 0 and 2, onto fma(q1, d1, rn(p0)) in column 1, and entry (2, 2) is fma(q2, d2, rn(rn(p0) + rn(p1))).  The same
// expression at a second site is contracted differently again (it was tried: 1 ulp apart in entry (0, 1)), so this site spells
// the dense kernel's operations out; the dense kernel stays as it is, and tests/test_gpu_views_compact.py compares the two bit
// for bit on every shape, which is what notices a compiler that changes its mind.
__device__ __forceinline__ void view_compose_pinned(const float (&q)[9], const float* d, float* o)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p0 = q[a * 3] * d[c * 3], p1 = q[a * 3 + 1] * d[c * 3 + 1];
            const float inner = (a == 2 && c == 2) ? p0 + p1 : c == 1 ? fmaf(q[a * 3 + 1], d[c * 3 + 1], p0) : fmaf(q[a * 3], d[c * 3], p1);
            o[a * 3 + c] = fmaf(q[a * 3 + 2], d[c * 3 + 2], inner);
        }
}

}  // namespace ahv
