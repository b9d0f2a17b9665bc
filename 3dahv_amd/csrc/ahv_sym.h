// ahv_sym.h -- pose selection modulo an object's symmetry group: the symmetric trace and its maximiser, ONE copy of the maths for
// the fold (sym_fold_kernel) and the symmetric mode selection (topk_modes_sym_kernel) in ahv_select.hip (tile rule: ahv_tile.h).
//
// Hypotheses are relative rotations R (source view -> target view); the group, written in the source view's frame, acts on the
// right: R and R S are the same pose.  A group is G <= kSymMaxG matrices S_g (S_0 the identity, exactly) and, optionally, a unit
// axis a about which every rotation is a symmetry as well; every S_g then maps a to sigma_g a, sigma_g = +-1.
//     t_G(R, A) = max over g (and phi) of  sum_ab (R S_g Rot(a, phi))[a][b] A[a][b]
//  - finite part: t_g = <R, A S_g^T>.  The G matrices T_g = A S_g^T are built ONCE per anchor (sym_orbit_matrix) into LDS and
//    read as broadcasts; a hypothesis pays nine FMAs per element, in the fmaf order of the plain modes kernel, and T_0 is A's own
//    bytes -- so the trivial group gives the plain trace bit for bit.
//  - with an axis: M = A^T R S_g, p = a^T M a, c = tr M - p, s = tr(M [a]x); the maximum over phi of tr(M Rot(a, phi)) =
//    p + c cos phi + s sin phi is p + h, h = sqrt(c^2 + s^2), at cos phi = c / h, sin phi = s / h (phi = 0 when h = 0): no
//    trigonometric call.  Because S_g [a]x = sigma_g [a]x S_g, all three are forms in the SAME table:
//        tr M = <R, T_g>,   p = sigma_g (A a) . (R a),   s = sigma_g <R [a]x, T_g>,
//    so an axis costs a second nine-FMA chain per element and R a, R [a]x once per hypothesis.
// The first maximiser wins (strict >, g ascending); a NaN value never replaces the incumbent, and a NaN t_0 stays: a NaN
// hypothesis or anchor has a NaN t_G, which is within nothing.
#pragma once

namespace ahv {

constexpr int kSymMaxG = 64;

// T = A S_g^T (LDS or registers); g == 0: A's bytes (S_0 is the identity by contract)
__device__ __forceinline__ void sym_orbit_matrix(const float* A, const float* Sg, int g, float* T)
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = fmaf(A[a * 3 + 2], Sg[c * 3 + 2], fmaf(A[a * 3 + 1], Sg[c * 3 + 1], A[a * 3] * Sg[c * 3]));
            T[a * 3 + c] = g == 0 ? A[a * 3 + c] : v;
        }
}

// sigma_g: +1 where S_g keeps the axis, -1 where it reverses it
__device__ __forceinline__ float sym_axis_sign(const float* Sg, const float (&a)[3])
{
    float d = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) d = fmaf(a[i], fmaf(Sg[i * 3 + 2], a[2], fmaf(Sg[i * 3 + 1], a[1], Sg[i * 3] * a[0])), d);
    return d < 0.0f ? -1.0f : 1.0f;
}

// y = A a
__device__ __forceinline__ void sym_apply(const float* A, const float (&a)[3], float* y)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = fmaf(A[i * 3 + 2], a[2], fmaf(A[i * 3 + 1], a[1], A[i * 3] * a[0]));
}

// t_G and its maximiser for kE hypotheses against one anchor (the table is read once for all of them).
//   r    the hypotheses;  T [G][9] the anchor's table (LDS), sig [G] (LDS) and Aa = A a (3 floats): used with kAxis only
//   t    t_G;  g  the first maximising element;  cphi, sphi  cos / sin of the maximising axis angle (1, 0 without an axis)
template <int kE, bool kAxis>
__device__ __forceinline__ void sym_trace(const float (&r)[kE][9], const float* T, int G, const float* sig, const float (&a)[3],
                                          const float* Aa, float (&t)[kE], int (&gs)[kE], float (&cphi)[kE], float (&sphi)[kE])
{
    float rk[kAxis ? kE : 1][9], pd[kAxis ? kE : 1];  // R [a]x and (A a) . (R a)
    float cc[kE], hh[kE];
    if constexpr (kAxis) {
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            float u[3];
            sym_apply(r[e], a, u);
            pd[e] = fmaf(Aa[2], u[2], fmaf(Aa[1], u[1], Aa[0] * u[0]));
#pragma unroll
            for (int i = 0; i < 3; ++i) {  // [a]x = [[0, -a2, a1], [a2, 0, -a0], [-a1, a0, 0]]
                rk[e][i * 3 + 0] = fmaf(r[e][i * 3 + 1], a[2], -(r[e][i * 3 + 2] * a[1]));
                rk[e][i * 3 + 1] = fmaf(r[e][i * 3 + 2], a[0], -(r[e][i * 3 + 0] * a[2]));
                rk[e][i * 3 + 2] = fmaf(r[e][i * 3 + 0], a[1], -(r[e][i * 3 + 1] * a[0]));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kE; ++e) {
        t[e] = 0.0f;
        gs[e] = 0;
        cc[e] = 1.0f;
        sphi[e] = 0.0f;
        hh[e] = 1.0f;
    }
    for (int g = 0; g < G; ++g) {
        float m[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = T[g * 9 + i];
        const float sg = kAxis ? sig[g] : 1.0f;
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            float tr = 0.0f;
#pragma unroll
            for (int i = 0; i < 9; ++i) tr = fmaf(r[e][i], m[i], tr);
            float val = tr, c = 1.0f, s = 0.0f, h = 1.0f;
            if constexpr (kAxis) {
                float sk = 0.0f;
#pragma unroll
                for (int i = 0; i < 9; ++i) sk = fmaf(rk[e][i], m[i], sk);
                const float p = sg * pd[e];
                s = sg * sk;
                c = tr - p;
                h = sqrtf(fmaf(c, c, s * s));
                val = p + h;
            }
            if (g == 0 || val > t[e]) {  // the first maximiser; false for a NaN value
                t[e] = val;
                gs[e] = g;
                cc[e] = c;
                sphi[e] = s;
                hh[e] = h;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kE; ++e) {
        const bool turn = kAxis && hh[e] > 0.0f;  // false for a NaN h
        cphi[e] = turn ? cc[e] / hh[e] : 1.0f;
        sphi[e] = turn ? sphi[e] / hh[e] : 0.0f;
    }
}

// Q = S_g Rot(a, phi), Rot = cos I + sin [a]x + (1 - cos) a a^T: the group element a hypothesis is folded by
template <bool kAxis>
__device__ __forceinline__ void sym_element(const float* Sg, const float (&a)[3], float cphi, float sphi, float (&Q)[9])
{
    if constexpr (!kAxis) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Q[i] = Sg[i];
    } else {
        const float k1 = 1.0f - cphi;
        const float rot[9] = {fmaf(k1 * a[0], a[0], cphi),         fmaf(k1 * a[0], a[1], -(sphi * a[2])), fmaf(k1 * a[0], a[2], sphi * a[1]),
                              fmaf(k1 * a[1], a[0], sphi * a[2]),  fmaf(k1 * a[1], a[1], cphi),           fmaf(k1 * a[1], a[2], -(sphi * a[0])),
                              fmaf(k1 * a[2], a[0], -(sphi * a[1])), fmaf(k1 * a[2], a[1], sphi * a[0]),  fmaf(k1 * a[2], a[2], cphi)};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Q[i * 3 + j] = fmaf(Sg[i * 3 + 2], rot[6 + j], fmaf(Sg[i * 3 + 1], rot[3 + j], Sg[i * 3] * rot[j]));
    }
}

}  // namespace ahv
