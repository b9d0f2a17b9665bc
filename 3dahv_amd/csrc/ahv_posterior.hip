// ahv_posterior.hip -- the pose posterior and the draws from it: softmax statistics of a scored set over anchor buckets
// (partial, merge, finish: masses, mean poses, spreads) and systematic resampling (a record per tile, the scan, the draws).
// fp64 sums in one fixed order, no float atomics: the same inputs give the same bytes.  The kernels walk the tile rule of
// ahv_tile.h and reduce with ahv_wave.h's wave sums and maxima.  Not here: the anchors' selection (the modes kernels) and the
// compose of the drawn hypotheses (compose_rotations_indexed_kernel), both in ahv_select.hip; the tracker's own resampling
// (ahv_track.hip).
#include "ahv_launch.h"
#include "ahv_tile.h"

namespace ahv {

// ---------------------------------------------------------------------------------
// Pose posterior (ahv_pose_posterior_f32 / _merge / _finish_f32): softmax statistics of the scored set at inverse temperature
// beta, split over K anchor buckets (hypothesis i belongs to the FIRST anchor k with t(i, k) >= tau, else to the rest).  What is
// kept per bucket and for the whole set is a RECORD of kPostRec doubles -- m (the largest score met, -inf when empty), and
// relative to it mass = sum w, S = sum w s, M = sum w R (9), w = exp((s - m) beta) -- so that two records merge by the
// online-softmax rule: m = max, each side rescaled by exp((m_side - m) beta).  A sample's STATE is a 16-byte header (int64
// n_excluded, int64 reserved) and K + 2 records: buckets 0 .. K-1, the rest bucket, the whole set.
//  - posterior_partial_kernel: ONE pass over scores and R on the grid rule of the modes kernels (tiles of kTopkTile, four
//    consecutive hypotheses per lane: load_scores4 / load_rotations4).  The anchors sit in LDS.  A lane keeps
//    online-softmax sums (fp32 weights, fp64 sums) for the whole set and the rest bucket; a mode bucket is hit rarely and is reduced wave-wide, only
//    when a ballot says some lane hit it, into the wave's LDS row in program order.  Wave sums are DPP row operations in fp64,
//    the four waves are combined in the order 0..3, one partial state per workgroup goes to the workspace.
//  - posterior_merge_kernel: states [P][B] -> state [B] in the order p = 0 .. P-1 (into the state, or from empty): the second
//    launch of a call and the merge after an all-gather.
//  - posterior_finish_kernel: a state -> the outputs; the rotation nearest to M is the top eigenvector of Horn's 4 x 4
//    quaternion matrix (the maximiser of sum R o M over SO(3) = U diag(1, 1, det(U V^T)) V^T), by cyclic Jacobi in fp64.
// No floating-point atomics: for a given (B, N, K) every sum is taken in one fixed order, so results are bitwise reproducible.
// ---------------------------------------------------------------------------------
constexpr int kPostMaxModes = 16;
constexpr int kPostRec = 12;      // doubles per record: m, mass, S, M[9]
constexpr int kPostHeader = 16;   // bytes: int64 n_excluded, int64 reserved (0)

__host__ __device__ constexpr size_t posterior_state_stride_dev(int K) { return (size_t)kPostHeader + (size_t)(K + 2) * kPostRec * sizeof(double); }
size_t posterior_state_stride(int K) { return posterior_state_stride_dev(K); }

constexpr int kPostMaxParts = 63;  // partial states per sample (the figure of the top-K lists)

int posterior_parts(int64_t N)
{
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    return (int)(tiles < kPostMaxParts ? tiles : kPostMaxParts);
}

struct PostAcc {  // one lane's online-softmax sums: the weights are fp32 (expf), the sums fp64 -- S / mass - m cancels, and an fp32
    float m;      // S would put its own rounding (times beta) into the entropy of a peaked distribution
    double mass, S, M[9];
};

__device__ __forceinline__ void post_clear(PostAcc& a)
{
    a.m = -INFINITY;
    a.mass = 0.0;
    a.S = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.M[i] = 0.0;
}

__device__ __forceinline__ void post_add(PostAcc& a, float s, const float* r, float beta)
{
    if (s > a.m) {  // a new maximum: rescale what is there (by 0 when nothing is: m = -inf)
        const double f = (double)expf((a.m - s) * beta);
        a.mass *= f;
        a.S *= f;
#pragma unroll
        for (int i = 0; i < 9; ++i) a.M[i] *= f;
        a.m = s;
    }
    const double w = (double)expf((s - a.m) * beta);
    a.mass += w;
    a.S = fma(w, (double)s, a.S);
#pragma unroll
    for (int i = 0; i < 9; ++i) a.M[i] = fma(w, (double)r[i], a.M[i]);
}

// dst <- dst merged with src (records of kPostRec doubles), dst's side first
__device__ __forceinline__ void post_merge(double* dst, const double* src, double beta)
{
    const double ma = dst[0], mb = src[0];
    const double m = mb > ma ? mb : ma;
    if (m == -INFINITY) return;  // both empty
    const double fa = ma == -INFINITY ? 0.0 : exp((ma - m) * beta), fb = mb == -INFINITY ? 0.0 : exp((mb - m) * beta);
    dst[0] = m;
#pragma unroll
    for (int i = 1; i < kPostRec; ++i) dst[i] = dst[i] * fa + src[i] * fb;
}

// the 64 lanes' sums as one record, merged into row (LDS) by lane 63.  Called by whole waves only.
__device__ __forceinline__ void post_wave_into(const PostAcc& a, double beta, double* row)
{
    const float mw = wave_max_f32_dpp(a.m);
    const double f = a.m == -INFINITY ? 0.0 : exp(((double)a.m - (double)mw) * beta);
    double rec[kPostRec];
    rec[0] = (double)mw;
    rec[1] = wave_sum_dpp_f64(f * a.mass);
    rec[2] = wave_sum_dpp_f64(f * a.S);
#pragma unroll
    for (int i = 0; i < 9; ++i) rec[3 + i] = wave_sum_dpp_f64(f * a.M[i]);
    if ((threadIdx.x & 63) == 63) post_merge(row, rec, beta);
}

__global__ __launch_bounds__(kTopkThreads) void posterior_partial_kernel(const float* __restrict__ scores, const float* __restrict__ R,
                                                                         long r_batch_stride, int B, long N,
                                                                         const float* __restrict__ anchors, int K, float tau,
                                                                         float beta, char* __restrict__ partial)
{
    __shared__ double rows[kTopkThreads / 64][kPostMaxModes + 2][kPostRec];  // per wave: buckets, rest, whole
    __shared__ float anc[kPostMaxModes][9];
    __shared__ int used[kPostMaxModes];  // an all-zero anchor is an empty slot: skipped by this flag, not by its value
    __shared__ int n_excl;
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.y;
    const double beta_d = (double)beta;
    for (int e = tid; e < (kTopkThreads / 64) * (kPostMaxModes + 2) * kPostRec; e += kTopkThreads)
        (&rows[0][0][0])[e] = (e % kPostRec) == 0 ? (double)-INFINITY : 0.0;
    if (tid < K * 9) (&anc[0][0])[tid] = anchors[(long)b * K * 9 + tid];
    if (tid == 0) n_excl = 0;
    __syncthreads();
    if (tid < K) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) any = any || anc[tid][i] != 0.0f;  // true for a NaN entry: its t then matches nothing
        used[tid] = any ? 1 : 0;
    }
    __syncthreads();

    const float* s = scores + (long)b * N;
    const float* Rb = R + (long)b * r_batch_stride;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    PostAcc whole, rest;
    post_clear(whole);
    post_clear(rest);
    int excluded = 0;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform over the workgroup: every lane takes every trip)
        const long n0 = t * kTopkTile + (long)tid * 4;
        float sc[4], r[4][9];
        int bk[4];  // K: rest, k < K: bucket k, -1: no such hypothesis / not in the scored set
        const bool every[4] = {true, true, true, true};  // every hypothesis that exists counts (a slot past N: zeros)
        load_scores4(s, n0, N, 0.0f, sc);
        load_rotations4(Rb, n0, N, every, r);
        bool hit = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool exists = n0 + e < N;
            const bool scored = exists && fabsf(sc[e]) < __builtin_inff();  // false for NaN and +-inf
            excluded += (exists && !scored) ? 1 : 0;
            bk[e] = scored ? K : -1;
        }
        for (int k = K - 1; k >= 0; --k) {  // descending: the FIRST matching anchor is the one left standing
            if (!used[k]) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 9; ++i) acc = fmaf(r[e][i], anc[k][i], acc);
                bk[e] = (bk[e] >= 0 && acc >= tau) ? k : bk[e];  // false for a NaN t
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (bk[e] < 0) continue;
            post_add(whole, sc[e], r[e], beta);
            if (bk[e] == K) post_add(rest, sc[e], r[e], beta);
            else hit = true;
        }
        if (__ballot(hit)) {  // rare (a 15-degree cap holds 0.1 % of SO(3)); wave-uniform from here on
            for (int k = 0; k < K; ++k) {
                const bool mine = bk[0] == k || bk[1] == k || bk[2] == k || bk[3] == k;
                if (!__ballot(mine)) continue;
                PostAcc a;
                post_clear(a);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (bk[e] == k) post_add(a, sc[e], r[e], beta);
                post_wave_into(a, beta_d, rows[wave][k]);
            }
        }
    }
    post_wave_into(rest, beta_d, rows[wave][K]);
    post_wave_into(whole, beta_d, rows[wave][K + 1]);
    if (excluded) atomicAdd(&n_excl, excluded);  // an integer count: order does not matter
    __syncthreads();
    char* st = partial + ((size_t)blockIdx.x * B + b) * posterior_state_stride_dev(K);
    if (tid < K + 2) {  // the four waves in the order 0..3
        double rec[kPostRec];
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) rec[i] = rows[0][tid][i];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) post_merge(rec, rows[w][tid], beta_d);
        double* dst = reinterpret_cast<double*>(st + kPostHeader) + tid * kPostRec;
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) dst[i] = rec[i];
    }
    if (tid == 63) {
        reinterpret_cast<long long*>(st)[0] = n_excl;
        reinterpret_cast<long long*>(st)[1] = 0;
    }
}

// states [P][B] -> state [B], in the order p = 0 .. P-1; carry: state's own content comes first
__global__ __launch_bounds__(64) void posterior_merge_kernel(const char* __restrict__ states, int P, int B, int K, float beta,
                                                             char* __restrict__ state, bool carry)
{
    const int b = blockIdx.x, j = threadIdx.x;
    const size_t stride = posterior_state_stride_dev(K);
    char* dst = state + (size_t)b * stride;
    if (j < K + 2) {
        double* d = reinterpret_cast<double*>(dst + kPostHeader) + j * kPostRec;
        double rec[kPostRec];
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) rec[i] = carry ? d[i] : (i == 0 ? (double)-INFINITY : 0.0);
        for (int p = 0; p < P; ++p) {
            const double* src = reinterpret_cast<const double*>(states + ((size_t)p * B + b) * stride + kPostHeader) + j * kPostRec;
            double in[kPostRec];
#pragma unroll
            for (int i = 0; i < kPostRec; ++i) in[i] = src[i];
            post_merge(rec, in, (double)beta);
        }
#pragma unroll
        for (int i = 0; i < kPostRec; ++i) d[i] = rec[i];
    }
    if (j == 63) {
        long long n = carry ? reinterpret_cast<const long long*>(dst)[0] : 0;
        for (int p = 0; p < P; ++p) n += reinterpret_cast<const long long*>(states + ((size_t)p * B + b) * stride)[0];
        reinterpret_cast<long long*>(dst)[0] = n;
        reinterpret_cast<long long*>(dst)[1] = 0;
    }
}

// one Jacobi rotation of the symmetric A (4 x 4) in the (P, Q) plane, accumulated into V
template <int P, int Q>
__device__ __forceinline__ void jacobi4_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// Rm = the rotation nearest to M (Frobenius), spread = the angle whose cosine is (sum Rm o M - 1) / 2, in degrees.
// M is a weighted mean of the matrices (already divided by the mass).
__device__ __forceinline__ void post_project(const double* M, float* Rm, float* spread)
{
    double A[4][4] = {{M[0] + M[4] + M[8], M[7] - M[5], M[2] - M[6], M[3] - M[1]},
                      {M[7] - M[5], M[0] - M[4] - M[8], M[1] + M[3], M[2] + M[6]},
                      {M[2] - M[6], M[1] + M[3], -M[0] + M[4] - M[8], M[5] + M[7]},
                      {M[3] - M[1], M[2] + M[6], M[5] + M[7], -M[0] - M[4] + M[8]}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < 12; ++sweep) {  // cyclic Jacobi converges quadratically: 12 sweeps are far past fp64 for a 4 x 4
        jacobi4_rotate<0, 1>(A, V);
        jacobi4_rotate<0, 2>(A, V);
        jacobi4_rotate<0, 3>(A, V);
        jacobi4_rotate<1, 2>(A, V);
        jacobi4_rotate<1, 3>(A, V);
        jacobi4_rotate<2, 3>(A, V);
    }
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool take = A[c][c] > best;
        best = take ? A[c][c] : best;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = take ? V[k][c] : q[k];
    }
    const double nn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * nn, x = q[1] * nn, y = q[2] * nn, z = q[3] * nn;
    const double Rd[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                          2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                          2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) dot += Rd[i] * M[i];
    double cs = (dot - 1.0) * 0.5;
    cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;  // (a NaN stays a NaN)
    if (Rm) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Rm[i] = (float)Rd[i];
    }
    if (spread) *spread = (float)(acos(cs) * 57.295779513082320877);
}

// thread j of block b: bucket j < K, the rest bucket (j = K) or the whole set (j = K + 1)
__global__ __launch_bounds__(64) void posterior_finish_kernel(const char* __restrict__ state, int B, int K, float beta,
                                                              float* __restrict__ log_z, float* __restrict__ entropy,
                                                              float* __restrict__ mean_score, long long* __restrict__ n_excluded,
                                                              float* __restrict__ mode_prob, float* __restrict__ rest_prob,
                                                              float* __restrict__ mode_R_mean, float* __restrict__ R_mean,
                                                              float* __restrict__ mode_spread, float* __restrict__ spread)
{
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= K + 2) return;
    const char* st = state + (size_t)b * posterior_state_stride_dev(K);
    const double* recs = reinterpret_cast<const double*>(st + kPostHeader);
    const double* all = recs + (K + 1) * kPostRec;
    const double* me = recs + j * kPostRec;
    const double bd = (double)beta, m_all = all[0], Z = all[1];
    const bool empty = !(me[1] > 0.0);  // an empty slot, a bucket without a member, an empty scored set
    if (j == K + 1) {
        if (n_excluded) n_excluded[b] = reinterpret_cast<const long long*>(st)[0];
        if (log_z) log_z[b] = empty ? -INFINITY : (float)(m_all * bd + log(Z));
        if (entropy) entropy[b] = empty ? __builtin_nanf("") : (float)(log(Z) - bd * (all[2] / Z - m_all));
        if (mean_score) mean_score[b] = empty ? __builtin_nanf("") : (float)(all[2] / Z);
    } else {
        const float p = empty ? 0.0f : (float)(me[1] * exp((me[0] - m_all) * bd) / Z);
        if (j == K) {
            if (rest_prob) rest_prob[b] = p;
            return;
        }
        if (mode_prob) mode_prob[(long)b * K + j] = p;
    }
    float* Rm = j <= K ? (mode_R_mean ? mode_R_mean + ((long)b * K + j) * 9 : nullptr) : (R_mean ? R_mean + (long)b * 9 : nullptr);
    float* sp = j <= K ? (mode_spread ? mode_spread + (long)b * K + j : nullptr) : (spread ? spread + b : nullptr);
    if (!Rm && !sp) return;
    if (empty) {
        if (Rm) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Rm[i] = 0.0f;
        }
        if (sp) *sp = __builtin_nanf("");
        return;
    }
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = me[3 + i] / me[1];
    post_project(M, Rm, sp);
}

// ---------------------------------------------------------------------------------
// Posterior resampling (ahv_resample_f32): M systematic (low-variance) draws from the softmax of a score row.  With m the
// largest finite score, w_i = exp((s_i - m) beta) for a finite s_i, else 0, C_i the inclusive prefix sum of w and Z = C_{N-1},
// draw j sits at t_j = (j + u) Z / M and returns the one i with C_{i-1} <= t_j < C_i.  Stated per HYPOTHESIS instead: i owns the
// slots [h_{i-1}, h_i), h_i = clamp(ceil(C_i M / Z - u), 0, M) -- the number of draws that sit below C_i.  What must hold
// whatever the rounding holds by construction: the boundaries are INTEGERS, clamped tile by tile into the tile's own range,
// made non-decreasing by an integer max-scan, and the last hypothesis with a positive weight takes the range's end; a
// hypothesis without weight takes the boundary of the one before it and owns nothing.  Every slot then has exactly one owner,
// the draw list is non-decreasing, and there is one fixed summation order per (B, N): bitwise reproducible, no atomics.
//  - resample_partial_kernel: per tile of kTopkTile hypotheses (load_scores4) the tile's own finite maximum m_t and
//    sum expf((s - m_t) beta) in fp64 (a lane's four in sequence, DPP inside a wave, the four waves in the order 0..3): one
//    record { m_t, sum_t } per TILE to the workspace.
//  - resample_scan_kernel: one wave per sample.  m = max m_t; q_t = sum_t exp((m_t - m) beta) in fp64; the exclusive prefix
//    P_t in the order t = 0 .. T-1 by one lane (a serial pass over T = N / 1024 records: meant for the N of a verify step);
//    the tile boundaries G_t = h(P_t), G_0 = 0 and G_t = M behind the last tile that holds weight.  P_t is a running sum of
//    non-negative terms and h is monotone in its argument, so G is non-decreasing as it comes.  Record t becomes { P_t, G_t }.
//  - resample_emit_kernel: a tile that owns no slot is skipped.  Otherwise the weights again, against m this time; the in-tile
//    inclusive scan in fp64 (a lane's four in sequence, a wave scan by shuffles, four wave totals through LDS); the integer
//    boundaries and their max-scan in the same shape; the tile's 1024 boundaries in LDS as int32.  Then the threads stride
//    over the tile's DRAWS j in [G_t, G_{t+1}), each finding its hypothesis by a binary search in LDS -- a peaked row, where
//    one hypothesis owns nearly all M slots, is written by all 256 lanes and not by one.  A sample without a finite score has
//    G = 0, M, M, ...: tile 0 writes -1 into every slot.
// The hand-over between the launches is the KERNEL BOUNDARY: no ticket, no workgroup waits on another one, no atomics.
// The quotient is taken as (C M) / Z and not as C (M / Z): where the weights are exactly 1 (equal scores) C M and Z are
// integers, the division is exact wherever its result is an integer, and the draw list is the exact-arithmetic one.
// ---------------------------------------------------------------------------------
constexpr int kResHeader = 32;  // bytes per sample in front of the records: doubles m, Z, u, reserved (0)
constexpr int kResRecord = 16;  // bytes per record; tiles + 1 records per sample

int64_t resample_tiles(int64_t N) { return (N + kTopkTile - 1) / kTopkTile; }
size_t resample_stride(int64_t N) { return (size_t)kResHeader + (size_t)(resample_tiles(N) + 1) * kResRecord; }

__device__ __forceinline__ bool res_finite(float s) { return fabsf(s) < __builtin_inff(); }  // false for NaN and +-inf

// the number of draws j in [0, M) with (j + u) Z / M < C, for 0 <= C <= Z (to rounding), Z > 0
__device__ __forceinline__ long long res_boundary(double C, double Md, double Z, double u, long long M)
{
    const double x = ceil(C * Md / Z - u);
    if (!(x > 0.0)) return 0;  // (also a NaN: cannot arise, stays in range)
    return x >= Md ? M : (long long)x;
}

__global__ __launch_bounds__(kTopkThreads) void resample_partial_kernel(const float* __restrict__ scores, long N, long tiles,
                                                                        float beta, char* __restrict__ ws, size_t stride)
{
    __shared__ float wm[kTopkThreads / 64];
    __shared__ double wsum[kTopkThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const float* s = scores + (long)b * N;
    double* rec = reinterpret_cast<double*>(ws + (size_t)b * stride + kResHeader);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform over the workgroup)
        float sc[4];
        load_scores4(s, t * kTopkTile + (long)tid * 4, N, -INFINITY, sc);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = (res_finite(sc[e]) && sc[e] > mx) ? sc[e] : mx;
        mx = wave_max_f32_dpp(mx);
        if (lane == 0) wm[wave] = mx;
        __syncthreads();
        float mt = wm[0];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) mt = wm[w] > mt ? wm[w] : mt;
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += res_finite(sc[e]) ? (double)expf((sc[e] - mt) * beta) : 0.0;
        acc = wave_sum_dpp_f64(acc);
        if (lane == 63) wsum[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            double sum = wsum[0];
#pragma unroll
            for (int w = 1; w < kTopkThreads / 64; ++w) sum += wsum[w];
            rec[2 * t] = (double)mt;
            rec[2 * t + 1] = sum;
        }
        __syncthreads();  // wm / wsum are free for the next tile
    }
}

// one wave per sample; u: [B] or nullptr
__global__ __launch_bounds__(64) void resample_scan_kernel(char* __restrict__ ws, size_t stride, long tiles, long long M,
                                                           float beta, const float* __restrict__ u)
{
    __shared__ long last_tile;
    const int lane = threadIdx.x, b = blockIdx.x;
    double* hdr = reinterpret_cast<double*>(ws + (size_t)b * stride);
    double* rec = hdr + kResHeader / 8;
    const double bd = (double)beta, Md = (double)M;
    double m = -INFINITY;
    for (long t = lane; t < tiles; t += 64) m = rec[2 * t] > m ? rec[2 * t] : m;
    m = wave_max_f64(m);
    for (long t = lane; t < tiles; t += 64) {  // q_t over sum_t
        const double mt = rec[2 * t];
        rec[2 * t + 1] = mt == -INFINITY ? 0.0 : rec[2 * t + 1] * exp((mt - m) * bd);
    }
    __syncthreads();
    float uv = u ? u[b] : 0.5f;
    uv = (uv >= 0.0f && uv < 1.0f) ? uv : 0.5f;  // false for a NaN
    double Z = 0.0;
    if (lane == 0) {  // the prefix in the order t = 0 .. T-1; P_t over m_t
        long last = -1;
        for (long t = 0; t < tiles; ++t) {
            const double q = rec[2 * t + 1];
            rec[2 * t] = Z;
            Z += q;
            last = q > 0.0 ? t : last;
        }
        rec[2 * tiles] = Z;
        hdr[0] = m;
        hdr[1] = Z;
        hdr[2] = (double)uv;
        hdr[3] = 0.0;
        last_tile = last;
    }
    __syncthreads();
    Z = hdr[1];
    const long last = last_tile;
    long long* G = reinterpret_cast<long long*>(rec);
    for (long t = lane; t <= tiles; t += 64)  // G_t over q_t
        G[2 * t + 1] = t == 0 ? 0 : t > last ? M : res_boundary(rec[2 * t], Md, Z, (double)uv, M);
}

__global__ __launch_bounds__(kTopkThreads) void resample_emit_kernel(const float* __restrict__ scores, long N, long tiles,
                                                                     float beta, long long M, const char* __restrict__ ws,
                                                                     size_t stride, long long* __restrict__ idx)
{
    __shared__ __attribute__((aligned(16))) int hb[kTopkTile];                  // the tile's boundaries: hypothesis i owns the slots [hb[i-1], hb[i])
    __shared__ double wtot[kTopkThreads / 64];     // the waves' weight
    __shared__ int wlast[kTopkThreads / 64], wh[kTopkThreads / 64];
    __shared__ key_t wkey[kTopkThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const float* s = scores + (long)b * N;
    const double* hdr = reinterpret_cast<const double*>(ws + (size_t)b * stride);
    const double* rec = hdr + kResHeader / 8;
    const long long* G = reinterpret_cast<const long long*>(rec);
    long long* out = idx + (long)b * M;
    const double md = hdr[0], Z = hdr[1], u = hdr[2], Md = (double)M;
    const float m = (float)md;  // (exact: it is a score)
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {  // (uniform over the workgroup)
        const long long g0 = G[2 * t + 1], g1 = G[2 * t + 3];
        if (g1 <= g0 || g0 < 0 || g1 > M) continue;  // the tile owns no slot (a workspace that is not the scan's: stay in bounds)
        if (md == -INFINITY) {  // no finite score in the sample: tile 0 owns every slot
            for (long long j = g0 + tid; j < g1; j += kTopkThreads) out[j] = -1;
            continue;
        }
        const long n0 = t * kTopkTile + (long)tid * 4;
        float sc[4];
        load_scores4(s, n0, N, -INFINITY, sc);
        double r[4];
        bool has[4];    // a weight above 0
        int mine = -1;  // this lane's last hypothesis with weight, as its place in the tile
        double run = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double w = res_finite(sc[e]) ? (double)expf((sc[e] - m) * beta) : 0.0;
            has[e] = w > 0.0;
            mine = has[e] ? tid * 4 + e : mine;
            run += w;
            r[e] = run;
        }
        double incl = run;  // the wave's inclusive scan of the lanes' totals
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(incl, off, 64);
            incl = lane >= off ? incl + o : incl;
        }
        double excl = __shfl_up(incl, 1, 64);
        excl = lane == 0 ? 0.0 : excl;
        const int wl = wave_max_int(mine);
        if (lane == 63) wtot[wave] = incl;
        if (lane == 0) wlast[wave] = wl;
        __syncthreads();
        double base = 0.0;
        int lastpos = wlast[0];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) {
            base = w <= wave ? base + wtot[w - 1] : base;
            lastpos = wlast[w] > lastpos ? wlast[w] : lastpos;
        }
        if (lastpos < 0) {
            // Slots, but no weight: every fp32 weight of the tile underflowed against m while its fp64 tile sum did not (scores
            // more than 87 / beta below the maximum, and u = 0 or a tile in front of all others).  The slots go to the tile's
            // largest finite score, which is where the exact weights put them.
            key_t k = kKeyEmpty;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const key_t c = res_finite(sc[e]) ? pack_key(sc[e], (unsigned)(tid * 4 + e)) : kKeyEmpty;
                k = c > k ? c : k;
            }
            k = wave_max_key_dpp(k);
            if (lane == 0) wkey[wave] = k;
            __syncthreads();
            k = wkey[0];
#pragma unroll
            for (int w = 1; w < kTopkThreads / 64; ++w) k = wkey[w] > k ? wkey[w] : k;
            const long long at = t * kTopkTile + (k == kKeyEmpty ? 0 : key_index(k));
            for (long long j = g0 + tid; j < g1; j += kTopkThreads) out[j] = at;
            __syncthreads();
            continue;
        }
        const double P = rec[2 * t];
        int h[4];  // (M < 2^31)
        int hrun = (int)g0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = tid * 4 + e;
            long long v = g0;  // without weight: the boundary of the one before (after the max-scan)
            if (i >= lastpos) {
                v = g1;
            } else if (has[e]) {
                v = res_boundary(P + (base + (excl + r[e])), Md, Z, u, M);
                v = v < g0 ? g0 : v > g1 ? g1 : v;
            }
            hrun = (int)v > hrun ? (int)v : hrun;
            h[e] = hrun;
        }
        int hin = hrun;  // the wave's inclusive max-scan of the lanes' last boundaries
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(hin, off, 64);
            hin = (lane >= off && o > hin) ? o : hin;
        }
        int hex = __shfl_up(hin, 1, 64);
        hex = lane == 0 ? (int)g0 : hex;
        if (lane == 63) wh[wave] = hin;
        __syncthreads();
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) hex = (w <= wave && wh[w - 1] > hex) ? wh[w - 1] : hex;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = h[e] > hex ? h[e] : hex;
        *reinterpret_cast<int4*>(hb + tid * 4) = make_int4(h[0], h[1], h[2], h[3]);
        __syncthreads();
        for (long long j = g0 + tid; j < g1; j += kTopkThreads) {  // the owner of slot j: the first i with hb[i] > j
            int lo = 0, hi = lastpos;  // (hb[lastpos] = g1 > j)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((long long)hb[mid] > j) hi = mid;
                else lo = mid + 1;
            }
            out[j] = t * kTopkTile + lo;
        }
        __syncthreads();  // hb and the wave words are free for the next tile
    }
}

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_posterior_merge(const void* states, int P, int B, int K, float beta, void* state, bool carry, hipStream_t stream)
{
    hipLaunchKernelGGL(posterior_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, static_cast<const char*>(states), P, B, K,
                       beta, static_cast<char*>(state), carry);
    return hipGetLastError();
}

hipError_t launch_posterior(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, const float* anchors,
                            int K, float tau, float beta, void* state, void* workspace, bool carry, hipStream_t stream)
{
    const int parts = posterior_parts(N);
    hipLaunchKernelGGL(posterior_partial_kernel, dim3((unsigned)parts, (unsigned)B), dim3(kTopkThreads), 0, stream, scores, R,
                       (long)r_batch_stride, B, (long)N, anchors, K, tau, beta, static_cast<char*>(workspace));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_posterior_merge(workspace, parts, B, K, beta, state, carry, stream);
}

hipError_t launch_posterior_finish(const void* state, int B, int K, float beta, float* log_z, float* entropy, float* mean_score,
                                   int64_t* n_excluded, float* mode_prob, float* rest_prob, float* mode_R_mean, float* R_mean,
                                   float* mode_spread_deg, float* spread_deg, hipStream_t stream)
{
    hipLaunchKernelGGL(posterior_finish_kernel, dim3((unsigned)B), dim3(64), 0, stream, static_cast<const char*>(state), B, K, beta,
                       log_z, entropy, mean_score, reinterpret_cast<long long*>(n_excluded), mode_prob, rest_prob, mode_R_mean,
                       R_mean, mode_spread_deg, spread_deg);
    return hipGetLastError();
}

hipError_t launch_resample(const float* scores, int B, int64_t N, float beta, int64_t M, const float* u, int64_t* idx,
                           void* workspace, hipStream_t stream)
{
    const int64_t tiles = resample_tiles(N);
    const size_t stride = resample_stride(N);
    const dim3 grid = tile_grid(N, B);
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(resample_partial_kernel, grid, dim3(kTopkThreads), 0, stream, scores, (long)N, (long)tiles, beta, ws, stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_scan_kernel, dim3((unsigned)B), dim3(64), 0, stream, ws, stride, (long)tiles, (long long)M, beta, u);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resample_emit_kernel, grid, dim3(kTopkThreads), 0, stream, scores, (long)N, (long)tiles, beta, (long long)M,
                       static_cast<const char*>(ws), stride, reinterpret_cast<long long*>(idx));
    return hipGetLastError();
}

}  // namespace ahv
