// ahv_track.hip -- pose tracking over a frame sequence: the particle filter's predict step (diffuse_rotations,
// predict_rotations, track_advance) and the two smoothers over the particle history, Viterbi (smooth_step, smooth_backtrace)
// and forward-backward marginals (marginal_step, marginal_smooth).  The smoothers share one pairwise pass over a frame's
// particles (pairwise_walk) and differ in what they accumulate.  The sets the filter tracks are scored by ahv_score.hip and
// resampled by ahv_posterior.hip; the Haar stream of the fresh slots is ahv_so3.h's, shared with the hypothesis generators.
#include "ahv_device.h"
#include "ahv_launch.h"
#include "ahv_so3.h"

namespace ahv {

// ---------------------------------------------------------------------------------
// Particle-filter predict step (ahv_diffuse_rotations_f32, include/ahv.h): one thread per slot (b, j) of the new set.
//   elite  j == 0 with a key: R[b][decode(key_b)] copied bit for bit
//   fresh  j >= M - n_fresh: rotation (step B + b) M + j of the Haar stream of seed ^ kFreshSeed
//   else   R[b][idx[b][j]] exp([w]x), w = sigma z clipped to max_angle, composed as unit quaternions and normalised, so that
//          a set fed back for thousands of steps stays on SO(3)
// The noise block of a slot is Philox(key = seed, counter = (j, b | step[47:32] << 16, kDiffuseTag, step[31:0])): a function of
// (seed, step mod 2^48, b, j) alone, and never a block of the Haar stream (word 2 differs).  `step` is read on the device.
// ---------------------------------------------------------------------------------
constexpr unsigned long long kFreshSeed = 0x9E3779B97F4A7C15ull;
constexpr unsigned kDiffuseTag = 0x444946u, kAdvanceTag = 0x414456u, kVelocityTag = 0x56454Cu;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }  // false for NaN

// Scales (x, y, z) so that its norm is <= limit (limit > 0; 0 means no limit) and returns the norm of the result.  2^-21 of
// room on both sides of the comparison: the rounded vector's exact norm stays <= limit.  A NaN norm is left alone.
__device__ __forceinline__ float clip_norm(float& x, float& y, float& z, float limit)
{
    float a = sqrtf(x * x + y * y + z * z);
    if (limit > 0.0f && a * 1.00000048f > limit) {
        const float s = (limit / a) * 0.99999952f;
        x *= s; y *= s; z *= s;
        a = sqrtf(x * x + y * y + z * z);
    }
    return a;
}

__device__ __forceinline__ void diffuse_slot(const long long* __restrict__ idx, const float* __restrict__ R, long r_batch_stride,
                                             long N, const key_t* __restrict__ best_key, long M, long n_fresh,
                                             unsigned long long seed, const long long* __restrict__ step, float sigma,
                                             float max_angle, float* __restrict__ out, float* __restrict__ omega)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const long b = blockIdx.y;
    const unsigned long long t = (unsigned long long)*step;
    const long i = b * M + j;
    float* o = out + i * 9;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
    if (j == 0 && best_key) {
        const key_t key = best_key[b];
        long n = key_index(key);
        n = (key == kKeyEmpty || n < 0 || n >= N) ? 0 : n;  // as compose_rotations_topk_kernel: stay in bounds
        const float* r = R + b * r_batch_stride + n * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = r[k];
    } else if (j >= M - n_fresh) {
        haar_rotation(seed ^ kFreshSeed, (t * (unsigned long long)gridDim.y + (unsigned long long)b) * (unsigned long long)M + (unsigned long long)j, o);
    } else {
        long n = idx ? (long)idx[i] : j % N;
        n = (n < 0 || n >= N) ? 0 : n;  // -1 (a sample without a finite score) or a foreign list: stay in bounds
        const float* r = R + b * r_batch_stride + n * 9;
        const float rr[9] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
        unsigned c[4] = {(unsigned)j, (unsigned)b | ((unsigned)(t >> 32) << 16), kDiffuseTag, (unsigned)t};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        float z0, z1, z2, z3;
        box_muller4(c, z0, z1, z2, z3);
        w0 = sigma * z0; w1 = sigma * z1; w2 = sigma * z2;
        clip_norm(w0, w1, w2, max_angle);
        compose_rotation_vector(rr, w0, w1, w2, o);
    }
    if (omega) {
        float* w = omega + i * 3;
        w[0] = w0; w[1] = w1; w[2] = w2;
    }
}

__global__ __launch_bounds__(256) void diffuse_rotations_kernel(const long long* __restrict__ idx, const float* __restrict__ R,
                                                                long r_batch_stride, long N, const key_t* __restrict__ best_key,
                                                                long M, long n_fresh, unsigned long long seed,
                                                                const long long* __restrict__ step, float sigma, float max_angle,
                                                                float* __restrict__ out, float* __restrict__ omega)
{
    diffuse_slot(idx, R, r_batch_stride, N, best_key, M, n_fresh, seed, step, sigma, max_angle, out, omega);
}

// ---------------------------------------------------------------------------------
// Constant-velocity predict step (ahv_predict_rotations_f32, include/ahv.h): a particle is (R, v), v its body-frame rotation
// vector per frame.  One thread per slot (b, j), as diffuse_rotations_kernel; slot classes in this precedence:
//   elite  j == 0 with a key: R and v of row decode(key_b) copied bit for bit
//   coast  j == 1 with a key and `coast`: R_n exp([v_n]x), no noise -- the constant-velocity prediction of the previous arg-max
//   fresh  j >= M - n_fresh: the Haar rotation diffuse_rotations_kernel writes for the same (seed, step, b, j), v = 0
//   else   v' = damping v_i + sigma_vel y (clipped to max_speed), w = v' + sigma z (the second term clipped to max_angle),
//          out = R_i exp([w]x) composed as unit quaternions and normalised, exactly as diffuse_rotations_kernel does
// z is the block diffuse_rotations_kernel draws (third counter word kDiffuseTag), y a second block (kVelocityTag).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void predict_slot(const long long* __restrict__ idx, const float* __restrict__ R, long r_batch_stride,
                                             const float* __restrict__ V, long v_batch_stride, long N,
                                             const key_t* __restrict__ best_key, long M, long n_fresh, unsigned long long seed,
                                             const long long* __restrict__ step, float sigma, float sigma_vel, float damping,
                                             float max_angle, float max_speed, int coast, float* __restrict__ out,
                                             float* __restrict__ vel_out, float* __restrict__ omega)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const long b = blockIdx.y;
    const unsigned long long t = (unsigned long long)*step;
    const long i = b * M + j;
    float* o = out + i * 9;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    const bool elite = best_key && j == 0, coasting = best_key && j == 1 && coast;
    if (!elite && !coasting && j >= M - n_fresh) {
        haar_rotation(seed ^ kFreshSeed, (t * (unsigned long long)gridDim.y + (unsigned long long)b) * (unsigned long long)M + (unsigned long long)j, o);
    } else {
        long n;
        if (elite || coasting) {
            const key_t key = best_key[b];
            n = key_index(key);
            n = (key == kKeyEmpty || n < 0 || n >= N) ? 0 : n;  // as diffuse_rotations_kernel: stay in bounds
        } else {
            n = idx ? (long)idx[i] : j % N;
            n = (n < 0 || n >= N) ? 0 : n;
        }
        const float* r = R + b * r_batch_stride + n * 9;
        if (V) {
            const float* v = V + b * v_batch_stride + n * 3;
            v0 = v[0]; v1 = v[1]; v2 = v[2];
        }
        if (elite) {
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k] = r[k];
        } else {
            const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
            if (coasting) {
                w0 = v0; w1 = v1; w2 = v2;
            } else {
                const unsigned cb = (unsigned)b | ((unsigned)(t >> 32) << 16);
                unsigned c[4] = {(unsigned)j, cb, kVelocityTag, (unsigned)t};
                philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
                float y0, y1, y2, y3;
                box_muller4(c, y0, y1, y2, y3);
                v0 = fmaf(damping, v0, sigma_vel * y0); v1 = fmaf(damping, v1, sigma_vel * y1); v2 = fmaf(damping, v2, sigma_vel * y2);
                clip_norm(v0, v1, v2, max_speed);
                c[0] = (unsigned)j; c[1] = cb; c[2] = kDiffuseTag; c[3] = (unsigned)t;
                philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
                float z0, z1, z2, z3;
                box_muller4(c, z0, z1, z2, z3);
                float p0 = sigma * z0, p1 = sigma * z1, p2 = sigma * z2;
                clip_norm(p0, p1, p2, max_angle);
                w0 = v0 + p0; w1 = v1 + p1; w2 = v2 + p2;
            }
            const float rr[9] = {r00, r01, r02, r10, r11, r12, r20, r21, r22};
            compose_rotation_vector(rr, w0, w1, w2, o);
        }
    }
    float* vo = vel_out + i * 3;
    vo[0] = v0; vo[1] = v1; vo[2] = v2;
    if (omega) {
        float* w = omega + i * 3;
        w[0] = w0; w[1] = w1; w[2] = w2;
    }
}

__global__ __launch_bounds__(256) void predict_rotations_kernel(const long long* __restrict__ idx, const float* __restrict__ R,
                                                                long r_batch_stride, const float* __restrict__ V,
                                                                long v_batch_stride, long N, const key_t* __restrict__ best_key,
                                                                long M, long n_fresh, unsigned long long seed,
                                                                const long long* __restrict__ step, float sigma, float sigma_vel,
                                                                float damping, float max_angle, float max_speed, int coast,
                                                                float* __restrict__ out, float* __restrict__ vel_out,
                                                                float* __restrict__ omega)
{
    predict_slot(idx, R, r_batch_stride, V, v_batch_stride, N, best_key, M, n_fresh, seed, step, sigma, sigma_vel, damping, max_angle,
                 max_speed, coast, out, vel_out, omega);
}

// ---------------------------------------------------------------------------------
// Noise scale and fresh slots decided on the device (ahv_predict_rotations_ctl_f32 / ahv_track_control_f32, include/ahv.h).
// The control record of sample b is eight 32-bit words the caller owns; the predict step reads words 0-2 and the control step,
// one launch after select_rotation, rewrites all eight from what the frame showed.
// ---------------------------------------------------------------------------------
struct TrackControl {
    float sigma, sigma_vel;  // what the next predict step uses, radians
    int n_fresh;             // its fresh slots; any int: a reader clamps to [0, M]
    unsigned flags;          // kControlLost | kControlReacquired | kControlUpdated of the last decision
    float m;                 // running per-axis variance of the motion, rad^2
    float innovation;        // of the last decision, radians; NaN when not computed
    float score;             // the MAP score the last decision saw
    unsigned reserved;       // 0
};
static_assert(sizeof(TrackControl) == 4 * 8, "the record is AHV_TRACK_CONTROL_WORDS = 8 32-bit words (include/ahv.h)");
constexpr unsigned kControlLost = 1u, kControlReacquired = 2u, kControlUpdated = 4u;

// q(R) of a rotation matrix by Shepperd's branch, as compose_rotation_vector has it inline; unit up to rounding, either sign.
// A second copy on purpose: with that function calling this one the compiler scheduled the three kernels that compose
// differently (same instructions, another order), and their instruction sequences are pinned.
__device__ __forceinline__ void rotation_quaternion(const float (&r)[9], float& qr, float& qi, float& qj, float& qk)
{
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
}

__device__ __forceinline__ long clamp_fresh(int n_fresh, long M) { return n_fresh < 0 ? 0 : (n_fresh > M ? M : (long)n_fresh); }

// The predict step with sigma, sigma_vel and n_fresh of sample blockIdx.y read from its record: the slot functions of the two
// kernels above with those three values in the place of the launch arguments, so that a record holding the launch's values
// gives that kernel's bytes.  kWalk: diffuse_rotations_kernel's slots (no velocities, no coast slot, vel_out not written).
template <bool kWalk>
__global__ __launch_bounds__(256) void predict_rotations_ctl_kernel(const long long* __restrict__ idx, const float* __restrict__ R,
                                                                    long r_batch_stride, const float* __restrict__ V,
                                                                    long v_batch_stride, long N, const key_t* __restrict__ best_key,
                                                                    long M, const TrackControl* __restrict__ control,
                                                                    unsigned long long seed, const long long* __restrict__ step,
                                                                    float damping, float max_angle, float max_speed, int coast,
                                                                    float* __restrict__ out, float* __restrict__ vel_out,
                                                                    float* __restrict__ omega)
{
    const TrackControl* c = control + blockIdx.y;
    const float sigma = c->sigma, sigma_vel = c->sigma_vel;
    const long n_fresh = clamp_fresh(c->n_fresh, M);
    if constexpr (kWalk)
        diffuse_slot(idx, R, r_batch_stride, N, best_key, M, n_fresh, seed, step, sigma, max_angle, out, omega);
    else
        predict_slot(idx, R, r_batch_stride, V, v_batch_stride, N, best_key, M, n_fresh, seed, step, sigma, sigma_vel, damping,
                     max_angle, max_speed, coast, out, vel_out, omega);
}

// The control step: one thread per sample, no LDS, no atomics.  In this order (include/ahv.h states the contract):
//   nf          the record's n_fresh clamped to [0, M]: what the predict step of THIS frame used
//   reacquired  idx >= max(M - nf, first): the winner sits in a fresh slot
//   lost        !(score >= score_floor); a NaN score is lost
//   a           the innovation: the angle between P, the pose slot 0 (the previous MAP pose, bit for bit) coasts to, and the
//               winner R_cur[idx], as 2 atan2(|q_v|, |q_w|) of q = q(P)* q(R_cur[idx]) -- acos of a trace loses half the digits
//               near 0, where sigma_min lives.  NaN for an idx outside [0, M) and for a non-finite angle.
//   m           (1 - rate) m + rate a^2 / 3 unless lost, reacquired or a is NaN: a jump into a fresh slot is a re-acquisition, not
//               motion, and a lost track's innovation means nothing
//   sigma       lost ? sigma_max : clamp(gain sqrt(m), sigma_min, sigma_max); a NaN lands on sigma_min (fmaxf drops it)
//   sigma_vel   sigma_vel0 (sigma / sigma0);  n_fresh  lost ? n_fresh_lost : n_fresh0
__global__ __launch_bounds__(256) void track_control_kernel(const float* __restrict__ R_cur, const float* __restrict__ V_cur,
                                                            const long long* __restrict__ idx, const float* __restrict__ score, int B,
                                                            long M, long first, float sigma0, float sigma_vel0, int n_fresh0,
                                                            float sigma_min, float sigma_max, float gain, float rate,
                                                            float score_floor, int n_fresh_lost, TrackControl* __restrict__ control,
                                                            unsigned char* __restrict__ reacquired)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const TrackControl c = control[b];
    const long nf = clamp_fresh(c.n_fresh, M);
    const long long i = idx[b];
    const float s = score[b];
    const bool reacq = i >= (M - nf > first ? M - nf : first);
    const bool lost = !(s >= score_floor);
    float a = __builtin_nanf("");
    if (i >= 0 && i < M) {
        const float* r0 = R_cur + (long)b * M * 9;
        const float e[9] = {r0[0], r0[1], r0[2], r0[3], r0[4], r0[5], r0[6], r0[7], r0[8]};
        float p[9];
        if (V_cur) {
            const float* v = V_cur + (long)b * M * 3;
            compose_rotation_vector(e, v[0], v[1], v[2], p);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) p[k] = e[k];
        }
        const float* rw = r0 + i * 9;
        const float w[9] = {rw[0], rw[1], rw[2], rw[3], rw[4], rw[5], rw[6], rw[7], rw[8]};
        float pr, pi, pj, pk, wr, wi, wj, wk;
        rotation_quaternion(p, pr, pi, pj, pk);
        rotation_quaternion(w, wr, wi, wj, wk);
        // q(P)* q(R): Hamilton product with the first factor conjugated, the vector part as differences of paired products and
        // with no contraction: each difference of equal factors is exactly 0, so a winner that holds slot 0's bytes (no V) has
        // the innovation 0 and not a rounding residue of 1e-8.
        float qr, qi, qj, qk;
        {
#pragma clang fp contract(off)
            qr = pr * wr + pi * wi + pj * wj + pk * wk;
            qi = (pr * wi - pi * wr) + (pk * wj - pj * wk);
            qj = (pr * wj - pj * wr) + (pi * wk - pk * wi);
            qk = (pr * wk - pk * wr) + (pj * wi - pi * wj);
        }
        const float ang = 2.0f * atan2f(sqrtf(qi * qi + qj * qj + qk * qk), fabsf(qr));
        if (finite_f(ang)) a = ang;
    }
    const bool updated = !lost && !reacq && finite_f(a);
    const float m = updated ? (1.0f - rate) * c.m + rate * (a * a * (1.0f / 3.0f)) : c.m;
    const float sigma = lost ? sigma_max : fminf(fmaxf(gain * sqrtf(m), sigma_min), sigma_max);
    TrackControl n;
    n.sigma = sigma;
    n.sigma_vel = sigma_vel0 * (sigma / sigma0);
    n.n_fresh = lost ? n_fresh_lost : n_fresh0;
    n.flags = (lost ? kControlLost : 0u) | (reacq ? kControlReacquired : 0u) | (updated ? kControlUpdated : 0u);
    n.m = m;
    n.innovation = a;
    n.score = s;
    n.reserved = 0u;
    control[b] = n;
    reacquired[b] = reacq ? 1 : 0;
}

// Start of a tracker step (ahv_track_advance): u[b] of step t + 1, then the counter itself.  One workgroup: the barrier
// orders every read of *step before the one write.
__global__ __launch_bounds__(256) void track_advance_kernel(unsigned long long seed, long long* step, int B, float* __restrict__ u)
{
    const unsigned long long t1 = (unsigned long long)*step + 1ull;
    for (int b = threadIdx.x; b < B; b += 256) {
        unsigned c[4] = {(unsigned)b, (unsigned)(t1 >> 32), kAdvanceTag, (unsigned)t1};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        u[b] = (float)(c[0] >> 8) * (1.0f / 16777216.0f);  // 24 bits: [0, 1)
    }
    __syncthreads();
    if (threadIdx.x == 0) *step = (long long)t1;
}

// ---------------------------------------------------------------------------------
// What the smoothers share.  The particle history is a ring of H slots the caller owns, frame t in slot t mod H, each slot
// holding nb samples of M rows; every kernel below is launched with 256 threads.
// ---------------------------------------------------------------------------------
// First row of frame t of sample b.  int64: t may be past 2^32 (and t - 1 may be negative).
__device__ __forceinline__ long ring_row(long long t, long long H, long nb, long b, int M)
{
    return ((long)(((t % H) + H) % H) * nb + b) * (long)M;
}

// Pair step of a first arg-max over finite values: the larger value, then the lower index; (-inf, -1) stands for "none".
__device__ __forceinline__ void merge_first_max(float& v, int& i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// First arg-max of the workgroup: every thread brings the first maximum of its own finite candidates, or (-inf, -1), and
// every thread leaves with the workgroup's.  One barrier; part_v / part_i (four entries each) are read after it.
__device__ __forceinline__ void block_first_max(float& v, int& vi, float* part_v, int* part_i)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) merge_first_max(v, vi, __shfl_xor(v, s, 64), __shfl_xor(vi, s, 64));
    if (lane == 0) { part_v[wave] = v; part_i[wave] = vi; }
    __syncthreads();
    v = part_v[0]; vi = part_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) merge_first_max(v, vi, part_v[w], part_i[w]);
}

// ---------------------------------------------------------------------------------
// The pairwise pass of both smoothers: a workgroup owns kSmoothSucc = 16 "owner" rows j of one sample and splits the "other"
// rows i of a neighbouring frame 16 ways: lane l of wave w holds owner l mod 16 (its nine entries in registers) and belongs to
// group g = 4 w + l / 16.  The other rows go through LDS in tiles of 256 rows of 12 floats (nine entries, the row's log-weight
// minus the largest finite one m, two of padding: three 16-byte reads).  Thread k stages row k of a tile -- loaded into
// registers while the tile before is being walked -- and group g walks rows g, 16 + g, ..., 240 + g: the four groups of a wave
// read four adjacent rows, 192 contiguous bytes, so the reads of a 16-lane group broadcast and the four do not share a bank.
// A group meets its rows in increasing i and hands acc.add the candidate
//     x_ij = (lw_i - m) + max(-|other_i - r_j|_F^2 inv4s2, -jump)
// and i.  Every x_ij is one expression, evaluated once.  A row whose log-weight is not finite, and a row past the end of the
// set, is staged with NaN in place of lw_i - m: its x_ij is NaN, as is that of a NaN matrix, and the accumulator must pass
// over it.  m is found first, by the whole workgroup (one barrier); when no other row is alive the walk returns false there
// (the same in every thread) and has touched neither acc nor merge.  Otherwise every thread ends the walk with merge(): the
// reduction's own merge of the 16 partial results of an owner, which stays with the accumulator's kernel because its order is
// part of that reduction's contract.  It is called from here, on the path that walked, and not by the caller on the returned
// flag: written the second way the compiler carried the flag through the kernel (two more VGPRs in marginal_backward_kernel).
// The finite maximum is written out here for the same reason: as a function taking log_weight it cost the same two registers.
// ---------------------------------------------------------------------------------
constexpr int kSmoothSucc = 16, kSmoothTile = 256, kSmoothRow = 12;

template <class LogWeight, class Acc, class Merge>
__device__ __forceinline__ bool pairwise_walk(const float (&r)[9], const float* __restrict__ other, LogWeight log_weight, int M,
                                              float inv4s2, float jump, float* tile, float* wave_max, Acc& acc, Merge merge)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int group = 4 * wave + (lane >> 4);
    float m = -__builtin_inff();  // the largest finite log-weight (every workgroup of the sample finds the same one)
    for (long i = tid; i < M; i += 256) {
        const float d = log_weight(i);
        if (finite_f(d)) m = fmaxf(m, d);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if (lane == 0) wave_max[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    if (!finite_f(m)) return false;

    const float neg_jump = -jump;
    // this thread's row of a tile: nine entries and lw_i - m, NaN for a dead row and past the end
    float stage[10];
    const auto load_row = [&](long i) {
#pragma unroll
        for (int k = 0; k < 9; ++k) stage[k] = 0.0f;
        stage[9] = __builtin_nanf("");
        if (i < M) {
            const float* src = other + i * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) stage[k] = src[k];
            const float v = log_weight(i);
            if (finite_f(v)) stage[9] = v - m;
        }
    };
    load_row(tid);
    for (long i0 = 0; i0 < M; i0 += kSmoothTile) {
        __syncthreads();  // the previous tile has been read by every wave
        f32x4* dst = reinterpret_cast<f32x4*>(tile + tid * kSmoothRow);
        dst[0] = f32x4{stage[0], stage[1], stage[2], stage[3]};
        dst[1] = f32x4{stage[4], stage[5], stage[6], stage[7]};
        dst[2] = f32x4{stage[8], stage[9], 0.0f, 0.0f};
        __syncthreads();
        if (i0 + kSmoothTile < M) load_row(i0 + kSmoothTile + tid);  // in flight while this tile is walked
#pragma unroll 4
        for (int p = 0; p < kSmoothTile / 16; ++p) {
            const int row = 16 * p + group;
            const f32x4 a = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow);
            const f32x4 c = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 4);
            const f32x4 d = *reinterpret_cast<const f32x4*>(tile + row * kSmoothRow + 8);
            // ||other_i - r_j||_F^2 from the nine differences (3 - tr cancels for the near pairs that decide the result)
            const float e0 = a[0] - r[0], e1 = a[1] - r[1], e2 = a[2] - r[2], e3 = a[3] - r[3], e4 = c[0] - r[4];
            const float e5 = c[1] - r[5], e6 = c[2] - r[6], e7 = c[3] - r[7], e8 = d[0] - r[8];
            float q = e0 * e0;
            q = fmaf(e1, e1, q); q = fmaf(e2, e2, q); q = fmaf(e3, e3, q); q = fmaf(e4, e4, q);
            q = fmaf(e5, e5, q); q = fmaf(e6, e6, q); q = fmaf(e7, e7, q); q = fmaf(e8, e8, q);
            const float w = -(q * inv4s2);
            acc.add(d[1] + (w < neg_jump ? neg_jump : w), (int)i0 + row);  // (a NaN w stays NaN: fmaxf would drop it)
        }
    }
    merge();
    return true;
}

// ---------------------------------------------------------------------------------
// Trajectory smoothing over the particle history (ahv_smooth_step_f32 / ahv_smooth_backtrace_f32, include/ahv.h): a Viterbi
// recursion over the particle sets of the last H frames and the backtrace.
//
// Step: the owners are the successors j (the frame's own particles), the others the predecessors (the previous slot's
// predicted poses and deltas); a group keeps (max, first index) of its candidates c_ij, which no comparison selects when it is
// NaN.  The 16 partial results of a successor are merged by merge_first_max, four by lane shuffles and the waves' in LDS;
// (max, lowest index) does not depend on the order: the bytes do not depend on the split.  At M = 4 096 that is 256
// workgroups, one per CU, 256 pairs per lane.  The workgroup reads the previous slot only and writes its own rows of the
// current slot.
// ---------------------------------------------------------------------------------
struct FirstMax {
    float best = -__builtin_inff();
    int best_i = -1;
    __device__ __forceinline__ void add(float x, int i)
    {
        if (x > best) { best = x; best_i = i; }
    }
};

__global__ __launch_bounds__(256) void smooth_step_kernel(const float* __restrict__ R_cur, const float* __restrict__ scores,
                                                          const float* __restrict__ V_cur, const long long* __restrict__ step,
                                                          long long first_step, int M, long long H, float beta, float inv4s2,
                                                          float jump, float damping, float* __restrict__ hist_R,
                                                          float* __restrict__ hist_P, float* __restrict__ hist_delta,
                                                          int* __restrict__ hist_back)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_v[4][kSmoothSucc];
    __shared__ int part_i[4][kSmoothSucc];
    __shared__ float wave_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int succ = lane & (kSmoothSucc - 1);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long t = *step;
    const long row_cur = ring_row(t, H, nb, b, M), row_prev = ring_row(t - 1, H, nb, b, M);
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = R_cur + (b * (long)M + j) * 9;

    // hist_R[slot]: this workgroup's rows, bit for bit
    if (tid < rows * 9) hist_R[(row_cur + j0) * 9 + tid] = R_cur[(b * (long)M + j0) * 9 + tid];
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];

    FirstMax acc;
    bool has_prev = t > first_step;
    if (has_prev)
        has_prev = pairwise_walk(r, (hist_P ? hist_P : hist_R) + row_prev * 9, [&](long i) { return hist_delta[row_prev + i]; }, M,
                                 inv4s2, jump, tile, wave_max, acc, [&] {
            // the four groups of a wave (lanes succ, succ + 16, + 32, + 48), then the four waves
#pragma unroll
            for (int s = 16; s <= 32; s <<= 1)
                merge_first_max(acc.best, acc.best_i, __shfl_xor(acc.best, s, 64), __shfl_xor(acc.best_i, s, 64));
            if (lane < kSmoothSucc) { part_v[wave][lane] = acc.best; part_i[wave][lane] = acc.best_i; }
            __syncthreads();
        });
    float best = acc.best;
    int best_i = acc.best_i;

    if (tid < kSmoothSucc && live) {
        if (has_prev) {
#pragma unroll
            for (int w = 1; w < 4; ++w) merge_first_max(best, best_i, part_v[w][lane], part_i[w][lane]);
        }
        const float s = scores[b * (long)M + j];
        float delta = -__builtin_inff();
        int back = -1;
        if (finite_f(s)) {
            delta = beta * s;
            if (best_i >= 0) { delta += best; back = best_i; }
        }
        hist_delta[row_cur + j] = delta;
        hist_back[row_cur + j] = back;
    }
    if (hist_P && wave == 1 && lane < kSmoothSucc && live) {
        const float* v = V_cur + (b * (long)M + j) * 3;
        compose_rotation_vector(r, damping * v[0], damping * v[1], damping * v[2], hist_P + (row_cur + j) * 9);
    }
}

// Backtrace: one workgroup per sample walks t, t - 1, ... over F <= H frames and writes the outputs oldest first.  The index
// carried to the frame before is back[j]; with none carried (the start, or behind a break) the frame's first arg-max over its
// finite deltas is taken by the whole workgroup.  `carry` is the same in every thread, so the barriers are uniform.
__global__ __launch_bounds__(256) void smooth_backtrace_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_delta,
                                                               const int* __restrict__ hist_back, const long long* __restrict__ step,
                                                               long long first_step, int M, long long H, int F,
                                                               long long* __restrict__ path_idx, float* __restrict__ path_R)
{
    __shared__ float part_v[4];
    __shared__ int part_i[4];
    const int tid = threadIdx.x;
    const long b = blockIdx.x, nb = gridDim.x;
    const long long t = *step;
    int carry = -1;
    for (int k = 0; k < F; ++k) {
        const long long tk = t - k;
        const long o = b * (long)F + (F - 1 - k);
        long row = 0;
        if (tk < first_step) {
            carry = -1;  // never recorded
        } else {
            row = ring_row(tk, H, nb, b, M);
            if (carry < 0) {
                FirstMax own;
                for (long i = tid; i < M; i += 256) {
                    const float d = hist_delta[row + i];
                    if (finite_f(d)) own.add(d, (int)i);
                }
                block_first_max(own.best, own.best_i, part_v, part_i);
                __syncthreads();  // part_* are free for the next break
                carry = own.best_i;
            }
        }
        if (tid == 0) path_idx[o] = carry;
        if (tid < 9) path_R[o * 9 + tid] = carry >= 0 ? hist_R[(row + carry) * 9 + tid] : (tid % 4 == 0 ? 1.0f : 0.0f);
        if (carry >= 0) {
            const int nxt = hist_back[row + carry];
            carry = (nxt >= 0 && nxt < M) ? nxt : -1;  // a ring the step did not write: stay in bounds
        }
    }
}

// ---------------------------------------------------------------------------------
// Marginal smoothing over the same ring (ahv_marginal_step_f32 / ahv_marginal_smooth_f32, include/ahv.h): the sum-product
// recursions of the hidden-Markov model whose max-product recursion is smooth_step_kernel -- the same transition, the same
// pairwise_walk, log-sum-exp in place of max.  A lane keeps a running (max, sum) pair over the rows of its group, met in
// increasing index; a candidate that is NaN or -inf is skipped explicitly (expf(NaN) would poison the sum, where the Viterbi
// compare never selected it).  The pairs merge as (max, sum) pairs in a fixed order: lanes 16 apart, lanes 32 apart, then
// waves 1, 2, 3 onto wave 0 in LDS.  The running maximum is the data's own, not a fixed offset: with jump = +inf and far
// clusters every term may sit near -365 and still sum to a finite value.  Bitwise reproducible and independent of B; NOT
// independent of the split (a sum, unlike a max, depends on the order), so the 16 x 16 split of the rows is part of the
// contract.
//   forward   owners R_cur, others P/R and alpha of the previous slot: alpha_j = a_j + LSE_i[(alpha_i - m) + w_ij]
//   backward  owners P/R of slot tau, others R and g = emit + beta of slot tau + 1: beta_i = LSE_j[w_ij + (g_j - m')]
// ---------------------------------------------------------------------------------
// One more term of a running log-sum-exp, sum = sum_k exp(x_k - mx), from (-inf, 0).  x is finite: the caller skips NaN and -inf.
__device__ __forceinline__ void lse_add(float& mx, float& sum, float x)
{
    const float d = x - mx;  // +inf at the first term: e = 0, sum = 1
    const float e = expf(-fabsf(d));
    sum = d > 0.0f ? fmaf(sum, e, 1.0f) : sum + e;
    mx = fmaxf(mx, x);
}

// (max, sum) merge; an empty side is (-inf, 0).
__device__ __forceinline__ void lse_merge(float& mx, float& sum, float omx, float osum)
{
    const float nm = fmaxf(mx, omx);
    if (nm > -__builtin_inff()) {
        sum = sum * expf(mx - nm) + osum * expf(omx - nm);
        mx = nm;
    }
}

struct LogSumExp {
    float mx = -__builtin_inff(), sum = 0.0f;
    __device__ __forceinline__ void add(float x, int)
    {
        if (x > -__builtin_inff()) lse_add(mx, sum, x);  // (false for NaN)
    }
};

// The log-weight of other row i in both directions: a[i] + b[i], b == nullptr standing for zeros.  The sum is taken either
// way, so a -0.0f enters the forward step, which has no second term, as the +0.0f it is in the backward step.
struct SumOfTwo {
    const float* a;
    const float* b;
    __device__ __forceinline__ float operator()(long i) const { return a[i] + (b ? b[i] : 0.0f); }
};

// The 16 partial pairs of every owner after a pairwise_walk, merged in the contract's order; then threads 0..15 hold the pair
// of their owner, sum == 0 when no edge reaches it.
__device__ __forceinline__ void merge_owner_sums(LogSumExp& a, float (*part_m)[kSmoothSucc], float (*part_s)[kSmoothSucc])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the four groups of a wave (lanes succ, succ + 16, + 32, + 48), then the four waves
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1) {
        const float om = __shfl_xor(a.mx, s, 64), os = __shfl_xor(a.sum, s, 64);
        // both lanes of a pair must compute the same bytes: the lower lane's pair first
        if (lane & s) { float tm = om, ts = os; lse_merge(tm, ts, a.mx, a.sum); a.mx = tm; a.sum = ts; }
        else lse_merge(a.mx, a.sum, om, os);
    }
    if (lane < kSmoothSucc) { part_m[wave][lane] = a.mx; part_s[wave][lane] = a.sum; }
    __syncthreads();
    if (tid < kSmoothSucc) {
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(a.mx, a.sum, part_m[w][lane], part_s[w][lane]);
    }
}

// Forward step: alpha and emit of slot t mod H from the previous slot.  Reads hist_R / hist_P of slot t - 1 only.
__global__ __launch_bounds__(256) void marginal_step_kernel(const float* __restrict__ R_cur, const float* __restrict__ scores,
                                                            const long long* __restrict__ step, long long first_step, int M,
                                                            long long H, float beta, float inv4s2, float jump,
                                                            const float* __restrict__ hist_R, const float* __restrict__ hist_P,
                                                            float* __restrict__ hist_alpha, float* __restrict__ hist_emit)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_m[4][kSmoothSucc], part_s[4][kSmoothSucc], wave_max[4];
    const int tid = threadIdx.x, succ = tid & (kSmoothSucc - 1);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long t = *step;
    const long row_cur = ring_row(t, H, nb, b, M), row_prev = ring_row(t - 1, H, nb, b, M);
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = R_cur + (b * (long)M + j) * 9;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];
    LogSumExp acc;
    bool has_prev = t > first_step;
    if (has_prev) {
        has_prev = pairwise_walk(r, (hist_P ? hist_P : hist_R) + row_prev * 9, SumOfTwo{hist_alpha + row_prev, nullptr}, M, inv4s2,
                                 jump, tile, wave_max, acc, [&] { merge_owner_sums(acc, part_m, part_s); });
    }
    if (tid < kSmoothSucc && live) {
        const float s = scores[b * (long)M + j];
        float emit = -__builtin_inff(), alpha = -__builtin_inff();
        if (finite_f(s)) {
            emit = beta * s;
            if (!has_prev) alpha = emit;
            else if (acc.sum > 0.0f) alpha = emit + (acc.mx + logf(acc.sum));
        }
        hist_alpha[row_cur + j] = alpha;
        hist_emit[row_cur + j] = emit;
    }
}

// Backward step for frame tau = t - back, output column f = F - 1 - back: beta(tau) into logw[b][f] from slot tau + 1, whose
// beta is logw[b][f + 1] (zero for the newest frame, back == 1).  A frame before first_step is left to the finish kernel.
__global__ __launch_bounds__(256) void marginal_backward_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_P,
                                                                const float* __restrict__ hist_emit,
                                                                const long long* __restrict__ step, long long first_step, int M,
                                                                long long H, int F, int back, float inv4s2, float jump,
                                                                float* __restrict__ logw)
{
    __shared__ __attribute__((aligned(16))) float tile[kSmoothTile * kSmoothRow];
    __shared__ float part_m[4][kSmoothSucc], part_s[4][kSmoothSucc], wave_max[4];
    const int tid = threadIdx.x, succ = tid & (kSmoothSucc - 1);
    const long b = blockIdx.y, nb = gridDim.y;
    const long long tau = *step - back;
    if (tau < first_step) return;  // the whole workgroup
    const long row_own = ring_row(tau, H, nb, b, M), row_next = ring_row(tau + 1, H, nb, b, M);
    const int f = F - 1 - back;
    float* out = logw + (b * (long)F + f) * (long)M;
    const float* beta_next = back == 1 ? nullptr : out + M;
    const int j0 = blockIdx.x * kSmoothSucc;
    const int rows = min(kSmoothSucc, M - j0);
    const bool live = succ < rows;
    const int j = j0 + (live ? succ : 0);
    const float* rc = (hist_P ? hist_P : hist_R) + (row_own + j) * 9;
    float r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rc[k];
    LogSumExp acc;
    const bool has_next = pairwise_walk(r, hist_R + row_next * 9, SumOfTwo{hist_emit + row_next, beta_next}, M, inv4s2, jump, tile,
                                        wave_max, acc, [&] { merge_owner_sums(acc, part_m, part_s); });
    if (tid < kSmoothSucc && live) out[j] = !has_next ? 0.0f : (acc.sum > 0.0f ? acc.mx + logf(acc.sum) : -__builtin_inff());
}

// Finish: one workgroup per (sample, frame).  x_i = alpha_i + beta_i (beta = 0 in the newest frame), log gamma_i = x_i - LSE x
// written over beta, the first arg-max of the written values and its pose.  Thread k sums rows k, k + 256, ... in increasing
// order; the pairs merge lane by lane (xor 1, 2, ..., 32, the lower lane's pair first) and then wave by wave.
__global__ __launch_bounds__(256) void marginal_finish_kernel(const float* __restrict__ hist_R, const float* __restrict__ hist_alpha,
                                                              const long long* __restrict__ step, long long first_step, int M,
                                                              long long H, int F, float* __restrict__ logw,
                                                              long long* __restrict__ out_idx, float* __restrict__ out_R)
{
    __shared__ float part_m[4], part_s[4];
    __shared__ int part_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    const long b = blockIdx.y, nb = gridDim.y;
    const long long tau = *step - (F - 1 - f);
    const long o = b * (long)F + f;
    float* lw = logw + o * (long)M;
    const bool newest = f == F - 1;
    const float ninf = -__builtin_inff();
    long row = 0;
    FirstMax top;
    if (tau >= first_step) {
        row = ring_row(tau, H, nb, b, M);
        float mx = ninf, sum = 0.0f;
        for (long i = tid; i < M; i += 256) {
            const float x = hist_alpha[row + i] + (newest ? 0.0f : lw[i]);
            if (finite_f(x)) lse_add(mx, sum, x);
        }
#pragma unroll
        for (int s = 1; s <= 32; s <<= 1) {
            const float om = __shfl_xor(mx, s, 64), os = __shfl_xor(sum, s, 64);
            if (lane & s) { float tm = om, ts = os; lse_merge(tm, ts, mx, sum); mx = tm; sum = ts; }
            else lse_merge(mx, sum, om, os);
        }
        if (lane == 0) { part_m[wave] = mx; part_s[wave] = sum; }
        __syncthreads();
        mx = part_m[0]; sum = part_s[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(mx, sum, part_m[w], part_s[w]);
        __syncthreads();  // part_m is reused below
        if (sum > 0.0f) {
            const float log_z = mx + logf(sum);
            for (long i = tid; i < M; i += 256) {
                const float x = hist_alpha[row + i] + (newest ? 0.0f : lw[i]);
                const float g = finite_f(x) ? x - log_z : ninf;
                lw[i] = g;
                top.add(g, (int)i);  // increasing i: the first one of this thread; -inf is never taken
            }
            block_first_max(top.best, top.best_i, part_m, part_i);
        }
    }
    const int best_i = top.best_i;
    if (best_i < 0)
        for (long i = tid; i < M; i += 256) lw[i] = ninf;
    if (tid == 0) out_idx[o] = best_i;
    if (tid < 9) out_R[o * 9 + tid] = best_i >= 0 ? hist_R[(row + best_i) * 9 + tid] : (tid % 4 == 0 ? 1.0f : 0.0f);
}

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_diffuse_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const int64_t* best_key,
                                    int64_t M, int64_t n_fresh, int B, uint64_t seed, const int64_t* step, float sigma,
                                    float max_angle, float* out, float* omega, hipStream_t stream)
{
    hipLaunchKernelGGL(diffuse_rotations_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                       reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, (long)N,
                       reinterpret_cast<const key_t*>(best_key), (long)M, (long)n_fresh, (unsigned long long)seed,
                       reinterpret_cast<const long long*>(step), sigma, max_angle, out, omega);
    return hipGetLastError();
}

hipError_t launch_predict_rotations(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V,
                                    int64_t v_batch_stride, int64_t N, const int64_t* best_key, int64_t M, int64_t n_fresh, int B,
                                    uint64_t seed, const int64_t* step, float sigma, float sigma_vel, float damping,
                                    float max_angle, float max_speed, int coast, float* out, float* vel_out, float* omega,
                                    hipStream_t stream)
{
    hipLaunchKernelGGL(predict_rotations_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                       reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, V, (long)v_batch_stride, (long)N,
                       reinterpret_cast<const key_t*>(best_key), (long)M, (long)n_fresh, (unsigned long long)seed,
                       reinterpret_cast<const long long*>(step), sigma, sigma_vel, damping, max_angle, max_speed, coast, out,
                       vel_out, omega);
    return hipGetLastError();
}

hipError_t launch_predict_rotations_ctl(const int64_t* idx, const float* R, int64_t r_batch_stride, const float* V,
                                        int64_t v_batch_stride, int64_t N, const int64_t* best_key, int64_t M, const uint32_t* control,
                                        int B, uint64_t seed, const int64_t* step, float damping, float max_angle, float max_speed,
                                        int coast, float* out, float* vel_out, float* omega, hipStream_t stream)
{
    const dim3 grid((unsigned)((M + 255) / 256), (unsigned)B);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, V,
                           (long)v_batch_stride, (long)N, reinterpret_cast<const key_t*>(best_key), (long)M,
                           reinterpret_cast<const TrackControl*>(control), (unsigned long long)seed,
                           reinterpret_cast<const long long*>(step), damping, max_angle, max_speed, coast, out, vel_out, omega);
    };
    if (vel_out) launch(predict_rotations_ctl_kernel<false>);
    else launch(predict_rotations_ctl_kernel<true>);  // the walk: the caller passed neither V nor a coast slot
    return hipGetLastError();
}

hipError_t launch_track_control(const float* R_cur, const float* V_cur, const int64_t* idx, const float* score, int B, int64_t M,
                                int first, float sigma0, float sigma_vel0, int n_fresh0, float sigma_min, float sigma_max, float gain,
                                float rate, float score_floor, int n_fresh_lost, uint32_t* control, uint8_t* reacquired,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(track_control_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, R_cur, V_cur,
                       reinterpret_cast<const long long*>(idx), score, B, (long)M, (long)first, sigma0, sigma_vel0, n_fresh0, sigma_min,
                       sigma_max, gain, rate, score_floor, n_fresh_lost, reinterpret_cast<TrackControl*>(control), reacquired);
    return hipGetLastError();
}

hipError_t launch_track_advance(uint64_t seed, int64_t* step, int B, float* u, hipStream_t stream)
{
    hipLaunchKernelGGL(track_advance_kernel, dim3(1), dim3(256), 0, stream, (unsigned long long)seed,
                       reinterpret_cast<long long*>(step), B, u);
    return hipGetLastError();
}

hipError_t launch_smooth_step(const float* R_cur, const float* scores, const float* V_cur, const int64_t* step, int64_t first_step,
                              int B, int64_t M, int64_t H, float beta, float inv4s2, float jump, float damping, float* hist_R,
                              float* hist_P, float* hist_delta, int32_t* hist_back, hipStream_t stream)
{
    hipLaunchKernelGGL(smooth_step_kernel, dim3((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B), dim3(256), 0, stream,
                       R_cur, scores, V_cur, reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H,
                       beta, inv4s2, jump, damping, hist_R, hist_P, hist_delta, reinterpret_cast<int*>(hist_back));
    return hipGetLastError();
}

hipError_t launch_smooth_backtrace(const float* hist_R, const float* hist_delta, const int32_t* hist_back, const int64_t* step,
                                   int64_t first_step, int B, int64_t M, int64_t H, int64_t F, int64_t* path_idx, float* path_R,
                                   hipStream_t stream)
{
    hipLaunchKernelGGL(smooth_backtrace_kernel, dim3((unsigned)B), dim3(256), 0, stream, hist_R, hist_delta,
                       reinterpret_cast<const int*>(hist_back), reinterpret_cast<const long long*>(step), (long long)first_step,
                       (int)M, (long long)H, (int)F, reinterpret_cast<long long*>(path_idx), path_R);
    return hipGetLastError();
}

hipError_t launch_marginal_step(const float* R_cur, const float* scores, const int64_t* step, int64_t first_step, int B, int64_t M,
                                int64_t H, float beta, float inv4s2, float jump, const float* hist_R, const float* hist_P,
                                float* hist_alpha, float* hist_emit, hipStream_t stream)
{
    hipLaunchKernelGGL(marginal_step_kernel, dim3((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B), dim3(256), 0, stream,
                       R_cur, scores, reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, beta,
                       inv4s2, jump, hist_R, hist_P, hist_alpha, hist_emit);
    return hipGetLastError();
}

hipError_t launch_marginal_smooth(const float* hist_R, const float* hist_P, const float* hist_alpha, const float* hist_emit,
                                  const int64_t* step, int64_t first_step, int B, int64_t M, int64_t H, int64_t F, float inv4s2,
                                  float jump, float* logw, int64_t* idx, float* R, hipStream_t stream)
{
    const dim3 grid((unsigned)((M + kSmoothSucc - 1) / kSmoothSucc), (unsigned)B);
    for (int64_t back = 1; back < F; ++back) {
        hipLaunchKernelGGL(marginal_backward_kernel, grid, dim3(256), 0, stream, hist_R, hist_P, hist_emit,
                           reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, (int)F, (int)back,
                           inv4s2, jump, logw);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(marginal_finish_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, stream, hist_R, hist_alpha,
                       reinterpret_cast<const long long*>(step), (long long)first_step, (int)M, (long long)H, (int)F, logw,
                       reinterpret_cast<long long*>(idx), R);
    return hipGetLastError();
}

}  // namespace ahv
