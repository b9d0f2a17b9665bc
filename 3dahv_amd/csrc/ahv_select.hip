// ahv_select.hip -- pose selection: everything that happens AFTER the scores exist.  Packed keys (arg-max, fill), K-best
// lists (top-K, merge, decode + gather, compose), distinct modes -- plain and modulo a symmetry group, with the fold into a
// fundamental domain (ahv_sym.h) --, the pose posterior, draws from it (systematic resampling, the indexed compose) and the SO(3)
// ascent step.  These kernels
// read scores, keys and rotation matrices only: no volume, no MFMA.  (unpack_best_kernel, the decode without a gather, sits
// with the scorer in ahv_score.hip.)
#include "ahv_device.h"
#include "ahv_so3.h"
#include "ahv_sym.h"

namespace ahv {

// ---------------------------------------------------------------------------------
// arg-max over materialised scores (test_co3d.py:145), same packed key as the fused path.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ scores, int B, long N,
                                                     long n_offset, key_t* __restrict__ best_key)
{
    const int b = blockIdx.y;
    const float* s = scores + (long)b * N;
    key_t best = kKeyEmpty;
    for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
        const key_t k = pack_key(s[n], (unsigned)(n_offset + n));
        best = k > best ? k : best;
    }
    best = wave_max_key(best);
    if ((threadIdx.x & 63) == 0 && best != kKeyEmpty) atomicMax(best_key + b, best);
}

// best_key[0..B) = EMPTY (below every real key): one tiny launch, graph-capturable
__global__ void fill_keys_kernel(key_t* __restrict__ k, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) k[b] = kKeyEmpty;
}

// ---------------------------------------------------------------------------------
// K best hypotheses.  The single best is the list at K = 1: ahv_select_rotation_f32 and ahv_compose_rotations_f32 launch
// select_topk_kernel / compose_rotations_topk_kernel with K = 1 (argmax_kernel stays: one atomic max per wave, no list).
// A list is K packed keys in descending SIGNED order, distinct, padded with kKeyEmpty.  With pack_key as it is that order
// is torch.sort(scores, dim=1, descending=True, stable=True) truncated to K (NaN first, lowest index among equal
// scores, -0 = +0); it is NOT torch.topk's order, which leaves ties unspecified.
//
// Everything on the critical path stays inside ONE wave: no barrier and no LDS round trip per round.
//  - scores -> lists (topk_kernel<true>): a workgroup of four waves walks tiles of kTopkTile scores; a lane holds four
//    candidates (one 16-byte load), and each wave on its own runs K knock-out rounds over its 256 -- a wave-wide max by DPP
//    row operations, the lane that offered the winner moves to its largest key strictly below it -- and leaves a sorted
//    K-list in LDS.  The four wave lists and the workgroup's running list are then merged by counting ranks (a fresh
//    list: all keys distinct) or, when the caller's list is merged into in the same launch, by their HEADS.
//  - lists -> list (merge_heads): one lane per sorted list; a round is the wave-wide max of the heads, and every lane
//    whose head is the winner steps to its next entry (so a key met in several lists is taken once).  Up to 63 lists and
//    the running list per pass; more lists are taken in passes.  This is ahv_topk_merge_keys, and the second launch of
//    ahv_topk_f32.
// Order, distinctness and the tie rule fall out of the integer compare.  A sample's N scores are spread over up to
// kTopkMaxParts workgroups whose lists go to the workspace; the second launch merges them into the caller's list ACROSS A
// KERNEL BOUNDARY -- no ticket, no loads that must dodge a stale per-XCD L2 line.  N <= one tile: one launch, straight into
// the list.  (The first version ran every round workgroup-wide -- eight candidates per lane, four LDS words and a barrier
// per round, in both launches: 1.1 us per round and pair of launches, slower than torch.topk + gather at K = 64.)
// ---------------------------------------------------------------------------------
constexpr int kTopkThreads = 256;
constexpr int kTopkPerLane = 4;
constexpr int kTopkTile = kTopkThreads * kTopkPerLane;  // 1024 scores per tile
constexpr int kTopkMaxParts = 63;                       // partial lists per sample: with the running list, one lane each
constexpr int kTopkMaxK = 64;

// wave 0 only: merge sorted lists by their heads into out[0..K) (LDS).  mine: this lane's list (K keys, descending), or
// nullptr for a lane without one.
__device__ __forceinline__ void merge_heads(const key_t* mine, int K, key_t* out)
{
    const int lane = threadIdx.x & 63;
    int pos = 0;
    key_t head = mine ? mine[0] : kKeyEmpty;
    for (int r = 0; r < K; ++r) {
        const key_t m = wave_max_key_dpp(head);
        if (lane == 0) out[r] = m;
        if (m == kKeyEmpty) {  // fewer than K distinct keys: pad (uniform over the wave)
            for (int j = r + 1 + lane; j < K; j += 64) out[j] = kKeyEmpty;
            break;
        }
        while (head >= m) {  // my head won (or repeats the winner): step past it; kKeyEmpty < m ends the walk
            ++pos;
            head = pos < K ? mine[pos] : kKeyEmpty;
        }
    }
}

// one wave, K knock-out rounds over the lanes' candidates c[0..kTopkPerLane): out[0..K) (LDS) = the wave's sorted list
__device__ __forceinline__ void wave_knock_out(const key_t (&c)[kTopkPerLane], int K, key_t* out)
{
    const int lane = threadIdx.x & 63;
    key_t mine = c[0];
#pragma unroll
    for (int i = 1; i < kTopkPerLane; ++i) mine = c[i] > mine ? c[i] : mine;
    for (int r = 0; r < K; ++r) {
        const key_t m = wave_max_key_dpp(mine);
        if (lane == 0) out[r] = m;
        if (m == kKeyEmpty) {
            for (int j = r + 1 + lane; j < K; j += 64) out[j] = kKeyEmpty;
            break;
        }
        if (mine == m) {  // knocked out: my largest key strictly below the winner
            key_t nxt = kKeyEmpty;
#pragma unroll
            for (int i = 0; i < kTopkPerLane; ++i) nxt = (c[i] < m && c[i] > nxt) ? c[i] : nxt;
            mine = nxt;
        }
    }
}

// kScores: src = scores [B][N] (+ n_offset); workgroup (x, b) takes the tiles x, x + gridDim.x, ... of sample b.  Tiles are
// laid on the 16-byte grid of the sample's row (a = the row's misalignment in floats), so that a lane's four scores are
// one 16-byte load wherever all four exist; the ragged ends go element by element.
// !kScores: src = lists [N][B][K] (N lists per sample), every one sorted as a list is.
// carry: the list starts as out[b][0..K) (merge into) instead of empty.  out: [gridDim.x][B][K].
template <bool kScores>
__global__ __launch_bounds__(kTopkThreads) void topk_kernel(const void* __restrict__ src, int B, long N, long n_offset, int K,
                                                            key_t* __restrict__ out, bool carry)
{
    __shared__ key_t run[2][kTopkMaxK];  // the running list and the one being built
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    key_t* dst = out + ((long)blockIdx.x * B + b) * K;
    if (tid < K) run[0][tid] = carry ? dst[tid] : kKeyEmpty;
    int cur = 0;
    if constexpr (kScores) {
        __shared__ key_t wl[4][kTopkMaxK];  // the four wave lists of a tile
        const float* s = static_cast<const float*>(src) + (long)b * N;
        const long a = (long)((reinterpret_cast<unsigned long long>(s) >> 2) & 3ull);
        const long tiles = (N + a + kTopkTile - 1) / kTopkTile;
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            key_t c[kTopkPerLane];
            const long n0 = t * kTopkTile + (long)tid * 4 - a;  // first of the lane's four scores
            if (n0 >= 0 && n0 + 3 < N) {
                const float4 q = *reinterpret_cast<const float4*>(s + n0);
                c[0] = pack_key(q.x, (unsigned)(n_offset + n0));
                c[1] = pack_key(q.y, (unsigned)(n_offset + n0 + 1));
                c[2] = pack_key(q.z, (unsigned)(n_offset + n0 + 2));
                c[3] = pack_key(q.w, (unsigned)(n_offset + n0 + 3));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long n = n0 + e;
                    c[e] = (n >= 0 && n < N) ? pack_key(s[n], (unsigned)(n_offset + n)) : kKeyEmpty;
                }
            }
            wave_knock_out(c, K, wl[wave]);
            __syncthreads();  // the four wave lists (and, first time round, run[0]) are in LDS
            if (carry) {
                if (wave == 0) merge_heads(lane < 4 ? wl[lane] : lane == 4 ? run[cur] : nullptr, K, run[cur ^ 1]);
            } else {
                // A fresh list: the five lists hold keys of different hypotheses, all distinct, so a key's place in the
                // merged list is the number of keys above it -- counted by all 256 lanes at once instead of K more rounds.
                if (tid < K) run[cur ^ 1][tid] = kKeyEmpty;
                __syncthreads();
                for (int e = tid; e < 5 * K; e += kTopkThreads) {
                    const int l = e / K, j = e - l * K;
                    const key_t k = l < 4 ? wl[l][j] : run[cur][j];
                    if (k == kKeyEmpty) continue;
                    int rank = 0;
                    for (int i = 0; i < K; ++i)
                        rank += (wl[0][i] > k) + (wl[1][i] > k) + (wl[2][i] > k) + (wl[3][i] > k) + (run[cur][i] > k);
                    if (rank < K) run[cur ^ 1][rank] = k;
                }
            }
            cur ^= 1;
            __syncthreads();
        }
    } else {
        __shared__ key_t ls[kTopkMaxParts * kTopkMaxK];  // up to 63 lists of a pass
        const key_t* lists = static_cast<const key_t*>(src);
        for (long g0 = 0; g0 < N; g0 += kTopkMaxParts) {
            const int ng = (int)(N - g0 < kTopkMaxParts ? N - g0 : kTopkMaxParts);
            for (int e = tid; e < ng * K; e += kTopkThreads) {
                const int p = e / K;
                ls[e] = lists[((g0 + p) * B + b) * K + (e - p * K)];
            }
            __syncthreads();
            if (wave == 0) merge_heads(lane < ng ? ls + lane * K : lane == 63 ? run[cur] : nullptr, K, run[cur ^ 1]);
            cur ^= 1;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < K) dst[tid] = run[cur][tid];
}

// decode + gather in one launch, one thread per (b, k): (score, global index, R[idx]) of every slot of a list; at K = 1
// (best score, best index, R_pred = R[idx]) of test_co3d.py:145-146, for any number B of keys (a key's sample is its row of R
// only where R is per-sample).  An EMPTY slot gives -inf, -1 and a zero row; a slot owned by another shard a zero row.
// reset: the keys are handed back EMPTY, ready for the next verify step's atomic max (the step then needs no launch
// of its own to clear them: stream order puts this kernel between the two scorers).
// 256 threads per workgroup for every K: a verify step decodes a handful of slots (B * K, or 8 steps' keys at once), one
// workgroup whose idle waves retire at the bounds check; thousands of slots (a list per sample at B = 32) fill whole workgroups.
__global__ __launch_bounds__(256) void select_topk_kernel(key_t* __restrict__ keys, int K, const float* __restrict__ R,
                                                          long r_batch_stride, long n_offset, long N, int B,
                                                          float* __restrict__ R_out, float* __restrict__ scores_out,
                                                          long* __restrict__ idx_out, bool reset)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * K) return;
    const int b = (int)(i / K);
    const key_t k = keys[i];
    if (reset) keys[i] = kKeyEmpty;
    const long gidx = (k == kKeyEmpty) ? -1l : key_index(k);
    if (scores_out) scores_out[i] = (k == kKeyEmpty) ? -INFINITY : key_score(k);
    if (idx_out) idx_out[i] = gidx;
    if (R_out) {
        const long loc = gidx - n_offset;
        const bool mine = (k != kKeyEmpty) && loc >= 0 && loc < N;  // sharded: the owner rank holds the row, the others zeros
        const float* r = R + (long)b * r_batch_stride + (mine ? loc : 0) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) R_out[i * 9 + e] = mine ? r[e] : 0.0f;
    }
}

// Coarse-to-fine support (BASELINE.json configs[4]; build-defined, the reference scores one flat set): refinement hypotheses
// out[b][k * N2 + n] = R[idx_{b,k}] * D[n], where idx_{b,k} is decoded on the device from the packed keys of the coarse stage
// and D is a fixed set of small rotations.  Graph-capturable.  An EMPTY slot or one owned by another shard composes row 0.
__global__ __launch_bounds__(256) void compose_rotations_topk_kernel(const key_t* __restrict__ keys, int K,
                                                                     const float* __restrict__ R, long r_batch_stride,
                                                                     long n_offset, long N, const float* __restrict__ D,
                                                                     long N2, int B, float* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * K * N2) return;
    const long bk = i / N2;  // b * K + k
    const long n = i - bk * N2;
    const int b = (int)(bk / K);
    const key_t key = keys[bk];
    long idx = key_index(key) - n_offset;
    idx = (key == kKeyEmpty || idx < 0 || idx >= N) ? 0 : idx;  // empty slot / foreign shard: stay in bounds
    const float* r = R + (long)b * r_batch_stride + idx * 9;
    const float* d = D + n * 9;
    float* o = out + i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = r[a * 3] * d[c] + r[a * 3 + 1] * d[3 + c] + r[a * 3 + 2] * d[6 + c];
}

// ---------------------------------------------------------------------------------
// A lane's four consecutive hypotheses n0 .. n0 + 3 (grid rule of topk_modes_kernel and posterior_partial_kernel: tiles of
// kTopkTile hypotheses, 256 threads, tile t starts at hypothesis t * kTopkTile, n0 = t * kTopkTile + 4 tid).
//  - alignment rule: 16-byte loads only where THAT ADDRESS is 16-byte aligned.  A sample's score row starts at s + b N and a
//    per-sample R row at R + 9 b N: with N % 4 != 0 they start mid-vector, so the tile index says nothing about alignment.
//  - ragged-end rule: a lane whose four hypotheses do not all exist (n0 + 3 >= N) goes element by element and reads no slot
//    at or past N.
// (topk_kernel<true> does not load through these: it shifts its tiles onto the row's 16-byte grid by a, so its lanes straddle
// the row's start as well as its end and its vector test is on n0, not on the address.)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0; }

// sc[e] = s[n0 + e], fill where hypothesis n0 + e does not exist
__device__ __forceinline__ void load_scores4(const float* __restrict__ s, long n0, long N, float fill, float (&sc)[4])
{
    if (n0 + 3 < N && aligned16(s + n0)) {
        const float4 q = *reinterpret_cast<const float4*>(s + n0);
        sc[0] = q.x; sc[1] = q.y; sc[2] = q.z; sc[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) sc[e] = n0 + e < N ? s[n0 + e] : fill;
    }
}

// r[e] = the matrix of hypothesis n0 + e (Rb: the sample's row of R).  The four matrices are 144 contiguous bytes: nine
// 16-byte loads for all four, whatever want says; element by element only the matrices that exist and are wanted are read,
// the others come back zero.
__device__ __forceinline__ void load_rotations4(const float* __restrict__ Rb, long n0, long N, const bool (&want)[4],
                                                float (&r)[4][9])
{
    const float* rp = Rb + n0 * 9;
    if (n0 + 3 < N && aligned16(rp)) {
        float4 q[9];
#pragma unroll
        for (int v = 0; v < 9; ++v) q[v] = reinterpret_cast<const float4*>(rp)[v];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int f = e * 9 + i;
                const float4 v = q[f >> 2];
                r[e][i] = (f & 3) == 0 ? v.x : (f & 3) == 1 ? v.y : (f & 3) == 2 ? v.z : v.w;
            }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 9; ++i) r[e][i] = (n0 + e < N && want[e]) ? rp[e * 9 + i] : 0.0f;
    }
}

// ---------------------------------------------------------------------------------
// Distinct pose modes (ahv_topk_modes_f32): greedy suppression by geodesic distance over the WHOLE scored set.  Entry j of
// the list is the largest key still alive; the winner then kills itself (by index, unconditionally) and every alive
// hypothesis i with t(i, w) = sum_ab R_i[a][b] R_w[a][b] >= tau (tau = 1 + 2 cos theta: for rotations "within theta of
// the winner").  A NaN t kills nothing.  K + 1 dependent launches: the list is filled EMPTY, round 0 packs the keys into the
// alive state, round j >= 1 applies winner j - 1 and reduces the largest survivor.  The KERNEL BOUNDARY is the hand-over of
// keys[j - 1]: no workgroup waits on another one.
// Alive state: the packed keys themselves, state[b][Ns] (Ns = N rounded up to 4) in the caller's workspace, kKeyEmpty =
// dead -- 8 bytes per hypothesis, read every round, written only where a hypothesis dies; the survivor's key needs no
// re-packing.  Four consecutive hypotheses per lane (load_scores4 / load_rotations4).  A lane whose four hypotheses are all
// dead reads no matrix; a wave of such lanes issues no load; element by element a dead hypothesis's matrix is not read.
// ---------------------------------------------------------------------------------
typedef long long i64x2 __attribute__((ext_vector_type(2)));

// the workgroup's largest key -> one atomicMax into *dst (skipped when nothing survives: *dst was filled kKeyEmpty)
__device__ __forceinline__ void modes_publish(key_t best, key_t* wl, key_t* dst)
{
    const key_t m = wave_max_key_dpp(best);
    if ((threadIdx.x & 63) == 0) wl[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        key_t r = wl[0];
#pragma unroll
        for (int w = 1; w < kTopkThreads / 64; ++w) r = wl[w] > r ? wl[w] : r;
        if (r != kKeyEmpty) atomicMax(dst, r);
    }
}

// kFirst: round 0 -- state = pack_key(scores), keys[b][0] = the arg-max key.  !kFirst: round j.
template <bool kFirst>
__global__ __launch_bounds__(kTopkThreads) void topk_modes_kernel(const float* __restrict__ scores, const float* __restrict__ R,
                                                                  long r_batch_stride, long N, long Ns, long n_offset, int K,
                                                                  int j, float tau, key_t* __restrict__ state,
                                                                  key_t* __restrict__ keys)
{
    __shared__ key_t wl[kTopkThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    key_t* st = state + (long)b * Ns;
    key_t* list = keys + (long)b * K;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    key_t best = kKeyEmpty;
    if constexpr (kFirst) {
        const float* s = scores + (long)b * N;
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const long n0 = t * kTopkTile + (long)tid * 4;
            if (n0 >= N) continue;
            float sc[4];
            load_scores4(s, n0, N, 0.0f, sc);
            key_t c[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) c[e] = n0 + e < N ? pack_key(sc[e], (unsigned)(n_offset + n0 + e)) : kKeyEmpty;
            // (the row is padded to Ns: all four slots exist; the padding is written dead)
            *reinterpret_cast<i64x2*>(st + n0) = i64x2{c[0], c[1]};
            *reinterpret_cast<i64x2*>(st + n0 + 2) = i64x2{c[2], c[3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) best = c[e] > best ? c[e] : best;
        }
        modes_publish(best, wl, list);
    } else {
        const key_t prev = list[j - 1];
        if (prev == kKeyEmpty) return;  // the alive set ran out: keys[j..K) stay EMPTY (uniform over the grid)
        const long widx = key_index(prev) - n_offset;
        if (widx < 0 || widx >= N) return;  // (cannot happen for a list this call built: stay in bounds regardless)
        const float* Rb = R + (long)b * r_batch_stride;
        float w[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) w[i] = Rb[widx * 9 + i];
        for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const long n0 = t * kTopkTile + (long)tid * 4;
            if (n0 >= N) continue;
            const i64x2 c01 = *reinterpret_cast<const i64x2*>(st + n0), c23 = *reinterpret_cast<const i64x2*>(st + n0 + 2);
            key_t c[4] = {c01.x, c01.y, c23.x, c23.y};
            if (c[0] == kKeyEmpty && c[1] == kKeyEmpty && c[2] == kKeyEmpty && c[3] == kKeyEmpty) continue;
            const bool alive[4] = {c[0] != kKeyEmpty, c[1] != kKeyEmpty, c[2] != kKeyEmpty, c[3] != kKeyEmpty};
            float r[4][9], tr[4];  // (tr of a dead slot is never looked at)
            load_rotations4(Rb, n0, N, alive, r);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 9; ++i) acc = fmaf(r[e][i], w[i], acc);
                tr[e] = acc;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (c[e] == kKeyEmpty) continue;
                if (tr[e] >= tau || n0 + e == widx) {  // false for a NaN trace; the winner goes by its index
                    st[n0 + e] = kKeyEmpty;
                    continue;
                }
                best = c[e] > best ? c[e] : best;
            }
        }
        modes_publish(best, wl, list + j);
    }
}

// ---------------------------------------------------------------------------------
// Pose selection modulo a symmetry group (ahv_topk_modes_sym_f32 / ahv_sym_fold_f32; the maths: ahv_sym.h).
//  - topk_modes_sym_kernel: round j >= 1 of the mode selection with t_G(R_i, R_w) in the place of t(i, w).  Round 0 and the list
//    fill are the plain ones (topk_modes_kernel<true> knows no rotation), as are the alive state, the workspace and the hand-over of
//    keys[j - 1] across the kernel boundary.  Every workgroup builds the winner's orbit R_w S_g^T (G matrices) in LDS first.
//  - sym_fold_kernel: ONE pass on the grid rule of the modes kernels.  A hypothesis takes the FIRST non-empty anchor k with
//    t_G(R_n, A_k) >= tau and becomes R_n S_g* Rot(a, phi*), the member of its orbit nearest that anchor; a body-frame velocity
//    follows as (S_g* Rot)^T v.  The K G tables A_k S_g^T sit in LDS.  A lane reads its own four matrices before it writes them, so
//    R_out may be R itself (per-sample R).  No atomics, no workspace: the same inputs give the same bytes.
// ---------------------------------------------------------------------------------
constexpr int kSymFoldMaxK = 16;

template <bool kAxis>
__global__ __launch_bounds__(kTopkThreads) void topk_modes_sym_kernel(const float* __restrict__ R, long r_batch_stride, long N, long Ns,
                                                                      long n_offset, int K, int j, float tau,
                                                                      const float* __restrict__ S, long s_batch_stride, int G,
                                                                      const float* __restrict__ axis, long axis_batch_stride,
                                                                      key_t* __restrict__ state, key_t* __restrict__ keys)
{
    __shared__ key_t wl[kTopkThreads / 64];
    __shared__ float T[kSymMaxG * 9];
    __shared__ float sig[kSymMaxG];
    const int tid = threadIdx.x, b = blockIdx.y;
    key_t* st = state + (long)b * Ns;
    key_t* list = keys + (long)b * K;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    const key_t prev = list[j - 1];
    if (prev == kKeyEmpty) return;  // the alive set ran out (uniform over the grid)
    const long widx = key_index(prev) - n_offset;
    if (widx < 0 || widx >= N) return;
    const float* Rb = R + (long)b * r_batch_stride;
    float w[9], a[3] = {0.0f, 0.0f, 0.0f}, wa[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = Rb[widx * 9 + i];
    if constexpr (kAxis) {
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] = axis[(long)b * axis_batch_stride + i];
        sym_apply(w, a, wa);
    }
    if (tid < G) {
        float sg[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) sg[i] = S[(long)b * s_batch_stride + tid * 9 + i];
        sym_orbit_matrix(w, sg, tid, T + tid * 9);
        if constexpr (kAxis) sig[tid] = sym_axis_sign(sg, a);
    }
    __syncthreads();
    key_t best = kKeyEmpty;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n0 = t * kTopkTile + (long)tid * 4;
        if (n0 >= N) continue;
        const i64x2 c01 = *reinterpret_cast<const i64x2*>(st + n0), c23 = *reinterpret_cast<const i64x2*>(st + n0 + 2);
        key_t c[4] = {c01.x, c01.y, c23.x, c23.y};
        if (c[0] == kKeyEmpty && c[1] == kKeyEmpty && c[2] == kKeyEmpty && c[3] == kKeyEmpty) continue;
        const bool alive[4] = {c[0] != kKeyEmpty, c[1] != kKeyEmpty, c[2] != kKeyEmpty, c[3] != kKeyEmpty};
        float r[4][9], tr[4], cp[4], sp[4];
        int gs[4];
        load_rotations4(Rb, n0, N, alive, r);
        sym_trace<4, kAxis>(r, T, G, sig, a, wa, tr, gs, cp, sp);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (c[e] == kKeyEmpty) continue;
            if (tr[e] >= tau || n0 + e == widx) {  // false for a NaN t_G; the winner goes by its index
                st[n0 + e] = kKeyEmpty;
                continue;
            }
            best = c[e] > best ? c[e] : best;
        }
    }
    modes_publish(best, wl, list + j);
}

// (R / R_out and V / V_out may be the same buffers: no __restrict__ on them)
template <bool kAxis>
__global__ __launch_bounds__(kTopkThreads) void sym_fold_kernel(const float* R, long r_batch_stride, long N,
                                                                const float* __restrict__ S, long s_batch_stride, int G,
                                                                const float* __restrict__ axis, long axis_batch_stride,
                                                                const float* __restrict__ anchors, int K, float tau, long keep,
                                                                const float* V, float* R_out, float* V_out, int* __restrict__ which,
                                                                int* __restrict__ elem, float* __restrict__ trace)
{
    __shared__ float T[kSymFoldMaxK * kSymMaxG * 9];  // A_k S_g^T, [k][g][9]
    __shared__ float Sl[kSymMaxG * 9];
    __shared__ float sig[kSymMaxG];
    __shared__ float Aa[kSymFoldMaxK][3];
    __shared__ int used[kSymFoldMaxK];  // an all-zero anchor is an empty slot (the posterior's convention)
    const int tid = threadIdx.x, b = blockIdx.y;
    const float* An = anchors + (long)b * K * 9;
    float a[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (kAxis) {
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] = axis[(long)b * axis_batch_stride + i];
    }
    for (int e = tid; e < G * 9; e += kTopkThreads) Sl[e] = S[(long)b * s_batch_stride + e];
    __syncthreads();
    for (int e = tid; e < K * G; e += kTopkThreads) {
        const int k = e / G, g = e - k * G;
        float ak[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) ak[i] = An[k * 9 + i];
        sym_orbit_matrix(ak, Sl + g * 9, g, T + e * 9);
    }
    if (tid < K) {
        float ak[9];
        bool any = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            ak[i] = An[tid * 9 + i];
            any = any || ak[i] != 0.0f;  // true for a NaN entry: its t_G then matches nothing
        }
        used[tid] = any ? 1 : 0;
        if constexpr (kAxis) sym_apply(ak, a, Aa[tid]);
    }
    if (kAxis && tid < G) sig[tid] = sym_axis_sign(Sl + tid * 9, a);
    __syncthreads();

    const float* Rb = R + (long)b * r_batch_stride;
    float* Ro = R_out + (long)b * N * 9;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n0 = t * kTopkTile + (long)tid * 4;
        if (n0 >= N) continue;
        float r[4][9];
        const bool every[4] = {true, true, true, true};
        load_rotations4(Rb, n0, N, every, r);
        int wh[4], el[4];
        float tt[4], cp[4], sp[4];
        bool open[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wh[e] = el[e] = -1;
            tt[e] = __builtin_nanf("");
            cp[e] = 1.0f;
            sp[e] = 0.0f;
            open[e] = n0 + e < N && n0 + e >= keep;
        }
        for (int k = 0; k < K; ++k) {
            if (!used[k]) continue;                                        // (uniform over the workgroup)
            if (!__ballot(open[0] || open[1] || open[2] || open[3])) break;  // (uniform over the wave)
            float t4[4], c4[4], s4[4];
            int g4[4];
            sym_trace<4, kAxis>(r, T + k * G * 9, G, sig, a, Aa[k], t4, g4, c4, s4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (open[e] && t4[e] >= tau) {  // the FIRST anchor within; false for a NaN t_G
                    wh[e] = k;
                    el[e] = g4[e];
                    tt[e] = t4[e];
                    cp[e] = c4[e];
                    sp[e] = s4[e];
                    open[e] = false;
                }
            }
        }
        float v[4][3], vo[4][3];
        const long vb = ((long)b * N + n0) * 3;
        const bool whole = n0 + 3 < N;
        if (V) {
            if (whole && aligned16(V + vb)) {
                float4 q[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) q[i] = reinterpret_cast<const float4*>(V + vb)[i];
#pragma unroll
                for (int f = 0; f < 12; ++f) {
                    const float4 x = q[f >> 2];
                    v[f / 3][f % 3] = (f & 3) == 0 ? x.x : (f & 3) == 1 ? x.y : (f & 3) == 2 ? x.z : x.w;
                }
            } else {
#pragma unroll
                for (int f = 0; f < 12; ++f) v[f / 3][f % 3] = n0 + f / 3 < N ? V[vb + f] : 0.0f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // the identity element without an axis turn: the input's bytes, not a product with the identity
            const bool moved = wh[e] >= 0 && (el[e] != 0 || (kAxis && !(sp[e] == 0.0f && cp[e] > 0.0f)));
            float Q[9], o[9];
            sym_element<kAxis>(Sl + (moved ? el[e] : 0) * 9, a, cp[e], sp[e], Q);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    o[i * 3 + c] = fmaf(r[e][i * 3 + 2], Q[6 + c], fmaf(r[e][i * 3 + 1], Q[3 + c], r[e][i * 3] * Q[c]));
#pragma unroll
            for (int i = 0; i < 9; ++i) r[e][i] = moved ? o[i] : r[e][i];
            if (V) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float x = fmaf(Q[6 + c], v[e][2], fmaf(Q[3 + c], v[e][1], Q[c] * v[e][0]));  // (Q^T v)[c]
                    vo[e][c] = moved ? x : v[e][c];
                }
            }
        }
        float* rp = Ro + n0 * 9;
        if (whole && aligned16(rp)) {
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                const int f = q * 4;
                reinterpret_cast<float4*>(rp)[q] = make_float4(r[f / 9][f % 9], r[(f + 1) / 9][(f + 1) % 9], r[(f + 2) / 9][(f + 2) % 9],
                                                               r[(f + 3) / 9][(f + 3) % 9]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    if (n0 + e < N) rp[e * 9 + i] = r[e][i];
        }
        if (V) {
            if (whole && aligned16(V_out + vb)) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int f = q * 4;
                    reinterpret_cast<float4*>(V_out + vb)[q] = make_float4(vo[f / 3][f % 3], vo[(f + 1) / 3][(f + 1) % 3],
                                                                           vo[(f + 2) / 3][(f + 2) % 3], vo[(f + 3) / 3][(f + 3) % 3]);
                }
            } else {
#pragma unroll
                for (int f = 0; f < 12; ++f)
                    if (n0 + f / 3 < N) V_out[vb + f] = vo[f / 3][f % 3];
            }
        }
        const long ob = (long)b * N + n0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (n0 + e >= N) continue;
            if (which) which[ob + e] = wh[e];
            if (elem) elem[ob + e] = el[e];
            if (trace) trace[ob + e] = tt[e];
        }
    }
}

// ---------------------------------------------------------------------------------
// Multi-view verification (ahv_view_rotations_f32 / ahv_fuse_view_scores_f32): V posed reference views of one object, one
// query whose rotation is wanted, N hypotheses Q_n of it.  View v (absolute rotation A_v) sees hypothesis n as the relative
// rotation R_{v,n} = Q_n A_v^T (gt_src_2_tgt_R = R_tgt R_src^-1), the scorer gives s_{v,n}, and
//     S_n = (sum_v g_{v,n} w_v s_{v,n}) / (sum_v g_{v,n} w_v),   g_{v,n} = [w_v > 0] [no limit or t(Q_n, A_v) >= tau],
// summed over v = 0 .. V-1 in that order in fp32, the product rounded before the add; -inf when no view participates.  A view
// with w_v = 0 is never read; a NaN t does not participate; a participating NaN score makes S_n NaN.
//  - view_rotations_kernel: the composition, one thread per output matrix, laid out as the scorer's per-sample set of B V samples.
//  - fuse_views_kernel: ONE pass over scores [B][V][N] (and Q, only under an angle limit) on the grid rule of the modes kernels
//    (tiles of kTopkTile, four consecutive hypotheses per lane: load_scores4 / load_rotations4 -- a view's row starts at
//    s + (b V + v) N, mid-vector when N % 4 != 0).  A[b][.] and the weights sit in LDS; the weights arrive BY VALUE in the kernel
//    arguments, so a launch reads no host memory.  The packed key of S_n is reduced per workgroup (modes_publish: DPP inside a
//    wave, LDS across the four, one atomicMax per workgroup and sample) into the caller's key.  No float atomics: for given
//    inputs every sum is taken in one fixed order.
// ---------------------------------------------------------------------------------
constexpr int kViewsMax = 16;

struct ViewWeights {
    float w[kViewsMax];
};

// t(Q_n, A_v) = sum_ab Q_n[a][b] A_v[a][b]: ONE fp32 fmaf chain in one order for every kernel that decides participation
__device__ __forceinline__ float view_trace(const float (&q)[9], const float* a)
{
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) acc = fmaf(q[i], a[i], acc);
    return acc;
}

__global__ __launch_bounds__(256) void view_rotations_kernel(const float* __restrict__ Q, long q_batch_stride,
                                                             const float* __restrict__ A, int V, long N, long total,
                                                             float* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (b V + v) N + n
    if (i >= total) return;
    const long bv = i / N;
    const long n = i - bv * N;
    const long b = bv / V;
    const float* q = Q + b * q_batch_stride + n * 9;
    const float* d = A + bv * 9;  // A_v: column c of A_v^T is row c of A_v
    float* o = out + i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = q[a * 3] * d[c * 3] + q[a * 3 + 1] * d[c * 3 + 1] + q[a * 3 + 2] * d[c * 3 + 2];
}

__global__ __launch_bounds__(kTopkThreads) void fuse_views_kernel(const float* __restrict__ scores, const float* __restrict__ Q,
                                                                  long q_batch_stride, const float* __restrict__ A,
                                                                  const ViewWeights weights, int V, long N, long n_offset,
                                                                  float tau, bool limit, float* __restrict__ fused,
                                                                  key_t* __restrict__ best_key)
{
#pragma clang fp contract(off)  // w s is rounded before it is added: the definition's operation order
    __shared__ key_t wl[kTopkThreads / 64];
    __shared__ float Al[kViewsMax][9];
    __shared__ float wv[kViewsMax];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (limit && tid < V * 9) (&Al[0][0])[tid] = A[(long)b * V * 9 + tid];  // (Q and A are not read without a limit)
    if (tid < V) wv[tid] = weights.w[tid];
    __syncthreads();
    const float* s = scores + (long)b * V * N;
    const float* Qb = limit ? Q + (long)b * q_batch_stride : nullptr;
    float* f = fused ? fused + (long)b * N : nullptr;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    key_t best = kKeyEmpty;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n0 = t * kTopkTile + (long)tid * 4;
        if (n0 >= N) continue;
        float r[4][9];
        if (limit) {
            const bool every[4] = {true, true, true, true};
            load_rotations4(Qb, n0, N, every, r);
        }
        float num[4] = {0.0f, 0.0f, 0.0f, 0.0f}, den[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int v = 0; v < V; ++v) {
            const float w = wv[v];
            if (!(w > 0.0f)) continue;  // an absent view: its scores are not read (uniform over the workgroup)
            float sc[4];
            load_scores4(s + (long)v * N, n0, N, 0.0f, sc);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool g = true;
                if (limit) g = view_trace(r[e], Al[v]) >= tau;  // false for a NaN t
                const float p = w * sc[e];
                num[e] = g ? num[e] + p : num[e];
                den[e] = g ? den[e] + w : den[e];
            }
        }
        float S[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            S[e] = den[e] > 0.0f ? num[e] / den[e] : -INFINITY;
            if (n0 + e < N) {
                const key_t k = pack_key(S[e], (unsigned)(n_offset + n0 + e));
                best = k > best ? k : best;
            }
        }
        if (f) {
            if (n0 + 3 < N && aligned16(f + n0)) {
                *reinterpret_cast<float4*>(f + n0) = make_float4(S[0], S[1], S[2], S[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n0 + e < N) f[n0 + e] = S[e];
            }
        }
    }
    modes_publish(best, wl, best_key + b);
}

// ---------------------------------------------------------------------------------
// The nearest views of a pose, and staging what belongs to them (ahv_nearest_views_f32 / ahv_gather_views_f32): a tracked
// particle cloud sits within a few degrees of one pose, so only the K reference views nearest that pose are scored.
//  - nearest_views_kernel: 16 lanes per sample, lane v holds A_v and t_v = view_trace(anchor, A_v) -- the chain that decides
//    participation in fuse_views_kernel, so "the K nearest" and "within the angle" agree to the bit.  The V values go through
//    LDS and lane v counts the views ranked ahead of it (t descending, the lower v first among equals, a NaN behind every
//    number): that count is its place, and the lanes with a place below K write their index and a bit copy of their matrix.
//    The anchor is read here, on the device: a replayed graph follows a pose that has moved.  No atomics.
//  - gather_views_kernel: dst[b][k] = src[b][view_idx[b][k]] as 16-byte bit copies; workgroup (row, chunk) reads its row's
//    index once (uniform), an index outside 0..V-1 gives a row of zeros, broadcast reads src[b] for every k.
// ---------------------------------------------------------------------------------
constexpr int kNearestThreads = 256;

__device__ __forceinline__ bool view_ranks_ahead(float tu, int u, float tv, int v)
{
    const bool nu = tu != tu, nv = tv != tv;
    if (nu || nv) return nu == nv ? u < v : nv;  // a number ranks ahead of a NaN; NaNs among themselves by v
    return tu > tv || (tu == tv && u < v);
}

__global__ __launch_bounds__(kNearestThreads) void nearest_views_kernel(const float* __restrict__ anchor,
                                                                        const float* __restrict__ A, int B, int V, int K,
                                                                        int* __restrict__ view_idx, float* __restrict__ A_sel)
{
    __shared__ float ts[kNearestThreads / kViewsMax][kViewsMax];
    const int tid = threadIdx.x, v = tid % kViewsMax, sl = tid / kViewsMax;
    const long b = (long)blockIdx.x * (kNearestThreads / kViewsMax) + sl;
    const bool live = b < B && v < V;
    float a[9];
    float t = 0.0f;
    if (live) {
        float q[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            q[i] = anchor[b * 9 + i];
            a[i] = A[(b * V + v) * 9 + i];
        }
        t = view_trace(q, a);
    }
    ts[sl][v] = t;
    __syncthreads();
    if (!live) return;
    int place = 0;
    for (int u = 0; u < V; ++u) place += (u != v && view_ranks_ahead(ts[sl][u], u, t, v)) ? 1 : 0;
    if (place >= K) return;
    view_idx[b * K + place] = v;
    float* o = A_sel + (b * K + place) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = a[i];
}

constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(kGatherThreads) void gather_views_kernel(const uint4* __restrict__ src, const int* __restrict__ view_idx,
                                                                      int V, int K, long L4, bool broadcast,
                                                                      uint4* __restrict__ dst)
{
    const long row = blockIdx.x;  // b K + k
    const long b = row / K;
    long from = b;
    if (!broadcast) {
        const int v = view_idx[row];
        from = (v >= 0 && v < V) ? b * V + v : -1;
    }
    uint4* d = dst + row * L4;
    const uint4* s = from >= 0 ? src + from * L4 : nullptr;
    for (long i = (long)blockIdx.y * kGatherThreads + threadIdx.x; i < L4; i += (long)gridDim.y * kGatherThreads)
        d[i] = s ? s[i] : make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------------------------
// Angle-limited multi-view verification, compact (ahv_view_rotations_compact_f32 / ahv_fuse_view_scores_compact_f32): under an
// angle limit only the pairs with g_{v,n} = [w_v > 0] [t(Q_n, A_v) >= tau] are composed and scored.  Per (b, v) the
// participating hypotheses are numbered in increasing n (a stable compaction): slot[b][v][n] = that number m while m < capacity,
// kViewSlotOverflow past it, kViewSlotExcluded for a pair that does not take part; out[b][v][m] = Q_n A_v^T, the identity in
// every slot past the list's end, so that out is the scorer's per-sample set of B V samples at N = capacity.
//  - view_compact_kernel<false>: workgroup (t, b) serves ALL V views of tile t (Q is read once): one count per (b, v, tile) to
//    the workspace.
//  - view_compact_kernel<true>: the same decision again (view_trace: the same bits), then the hand-over of the counts ACROSS
//    THE KERNEL BOUNDARY: a wave sums its views' tile counts -- those ahead of tile t and all of them (tiles integers per
//    view: 49 at N = 50 000; the sum is taken per workgroup, so the step costs tiles^2 loads per view and is meant for the N of
//    a verify step, not for 10^8).  Inside the tile a lane's rank is the ballot of the lanes below it, the popcount, and the
//    four wave totals in LDS.  The slot map, the composed matrices (view_compose_pinned), counts (tile 0) and the identity padding (workgroup t pads
//    the slots of ITS index range) follow.  With out = slot = NULL one workgroup per sample only sums: counts alone.
//  - fuse_views_compact_kernel: fuse_views_kernel with an int32 slot load and a gathered score load in place of the trace
//    test -- the same products, adds and division in the same order, hence the same bits for the same scores.  A slot outside
//    0 .. capacity-1 does not take part (no read behind the score row for a slot map that is not a compaction's).
// ---------------------------------------------------------------------------------
constexpr int kViewSlotExcluded = -1;
constexpr int kViewSlotOverflow = -2;

int64_t view_compact_tiles(int64_t N) { return (N + kTopkTile - 1) / kTopkTile; }

// sl[e] = slot[n0 + e], fill where hypothesis n0 + e does not exist (load_scores4's rules)
__device__ __forceinline__ void load_slots4(const int* __restrict__ s, long n0, long N, int fill, int (&sl)[4])
{
    if (n0 + 3 < N && aligned16(s + n0)) {
        const int4 q = *reinterpret_cast<const int4*>(s + n0);
        sl[0] = q.x; sl[1] = q.y; sl[2] = q.z; sl[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) sl[e] = n0 + e < N ? s[n0 + e] : fill;
    }
}

__device__ __forceinline__ int wave_sum_int(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// grid (tiles, B): one workgroup per tile and sample.  kEmit with out == nullptr: grid (1, B), counts only.
template <bool kEmit>
__global__ __launch_bounds__(kTopkThreads) void view_compact_kernel(const float* __restrict__ Q, long q_batch_stride,
                                                                    const float* __restrict__ A, const ViewWeights weights,
                                                                    int V, long N, long tiles, float tau, long capacity,
                                                                    int* __restrict__ tile_counts, float* __restrict__ out,
                                                                    int* __restrict__ slot, long long* __restrict__ counts)
{
    __shared__ float Al[kViewsMax][9];
    __shared__ float wv[kViewsMax];
    __shared__ int wt[kViewsMax][kTopkThreads / 64];  // participating pairs of view v in wave w of this tile
    __shared__ int ahead[kViewsMax], all[kViewsMax];  // ... in the tiles ahead of this one, in every tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const long t = blockIdx.x;
    if constexpr (kEmit) {
        for (int v = wave; v < V; v += kTopkThreads / 64) {  // (uniform over the wave)
            const int* tc = tile_counts + ((long)b * V + v) * tiles;
            int before = 0, every = 0;
            for (long i = lane; i < tiles; i += 64) {
                const int c = tc[i];
                every += c;
                before += i < t ? c : 0;
            }
            before = wave_sum_int(before);
            every = wave_sum_int(every);
            if (lane == 0) {
                ahead[v] = before;
                all[v] = every;
            }
        }
        if (!out) {  // count only (uniform over the grid)
            __syncthreads();
            if (tid < V) counts[(long)b * V + tid] = all[tid];
            return;
        }
    }
    if (tid < V * 9) (&Al[0][0])[tid] = A[(long)b * V * 9 + tid];
    if (tid < V) wv[tid] = weights.w[tid];
    __syncthreads();
    const long n0 = t * kTopkTile + (long)tid * 4;
    float r[4][9];
    const bool want[4] = {true, true, true, true};
    load_rotations4(Q + (long)b * q_batch_stride, n0, N, want, r);  // a lane past N reads nothing and holds zeros
    unsigned long long gm = 0ull;  // bit 4 v + e: view v takes part in hypothesis n0 + e
    for (int v = 0; v < V; ++v) {
        if (!(wv[v] > 0.0f)) continue;  // an absent view (uniform over the workgroup)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (n0 + e < N && view_trace(r[e], Al[v]) >= tau) gm |= 1ull << (4 * v + e);  // false for a NaN t
    }
    for (int v = 0; v < V; ++v) {
        int c = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) c += __popcll(__ballot((gm >> (4 * v + e)) & 1ull));
        if (lane == 0) wt[v][wave] = c;
    }
    __syncthreads();
    if constexpr (!kEmit) {
        if (tid < V) tile_counts[((long)b * V + tid) * tiles + t] = wt[tid][0] + wt[tid][1] + wt[tid][2] + wt[tid][3];
    } else {
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int v = 0; v < V; ++v) {
            const long bv = (long)b * V + v;
            long m = ahead[v];  // the slot of this lane's first participating hypothesis
            for (int w = 0; w < wave; ++w) m += wt[v][w];
            bool g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                g[e] = ((gm >> (4 * v + e)) & 1ull) != 0ull;
                m += __popcll(__ballot(g[e]) & below);  // the lanes below hold smaller n, whichever e
            }
            int sl[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sl[e] = kViewSlotExcluded;
                if (!g[e]) continue;
                sl[e] = m < capacity ? (int)m : kViewSlotOverflow;
                if (m < capacity) view_compose_pinned(r[e], Al[v], out + (bv * capacity + m) * 9);
                ++m;
            }
            int* srow = slot + bv * N;
            if (n0 + 3 < N && aligned16(srow + n0)) {
                *reinterpret_cast<int4*>(srow + n0) = make_int4(sl[0], sl[1], sl[2], sl[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n0 + e < N) srow[n0 + e] = sl[e];
            }
            // the identity in the slots of this workgroup's index range past the list's end (capacity <= N: every slot has a tile)
            const long end = (long)all[v] < capacity ? (long)all[v] : capacity;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long p = n0 + e;
                if (p < end || p >= capacity) continue;
                float* o = out + (bv * capacity + p) * 9;
#pragma unroll
                for (int i = 0; i < 9; ++i) o[i] = (i & 3) == 0 ? 1.0f : 0.0f;
            }
        }
        if (t == 0 && tid < V) counts[(long)b * V + tid] = all[tid];
    }
}

__global__ __launch_bounds__(kTopkThreads) void fuse_views_compact_kernel(const float* __restrict__ scores,
                                                                          const int* __restrict__ slot, const ViewWeights weights,
                                                                          int V, long N, long capacity, long n_offset,
                                                                          float* __restrict__ fused, key_t* __restrict__ best_key)
{
#pragma clang fp contract(off)  // w s is rounded before it is added: the definition's operation order
    __shared__ key_t wl[kTopkThreads / 64];
    __shared__ float wv[kViewsMax];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (tid < V) wv[tid] = weights.w[tid];
    __syncthreads();
    const float* s = scores + (long)b * V * capacity;
    const int* sm = slot + (long)b * V * N;
    float* f = fused ? fused + (long)b * N : nullptr;
    const long tiles = (N + kTopkTile - 1) / kTopkTile;
    key_t best = kKeyEmpty;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n0 = t * kTopkTile + (long)tid * 4;
        if (n0 >= N) continue;
        float num[4] = {0.0f, 0.0f, 0.0f, 0.0f}, den[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int v = 0; v < V; ++v) {
            const float w = wv[v];
            if (!(w > 0.0f)) continue;  // an absent view: neither its slots nor its scores are read (uniform over the workgroup)
            int sl[4];
            load_slots4(sm + (long)v * N, n0, N, kViewSlotExcluded, sl);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool g = sl[e] >= 0 && (long)sl[e] < capacity;
                const float sc = g ? s[(long)v * capacity + sl[e]] : 0.0f;  // slots rise with n: a near-coalesced gather
                const float p = w * sc;
                num[e] = g ? num[e] + p : num[e];
                den[e] = g ? den[e] + w : den[e];
            }
        }
        float S[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            S[e] = den[e] > 0.0f ? num[e] / den[e] : -INFINITY;
            if (n0 + e < N) {
                const key_t k = pack_key(S[e], (unsigned)(n_offset + n0 + e));
                best = k > best ? k : best;
            }
        }
        if (f) {
            if (n0 + 3 < N && aligned16(f + n0)) {
                *reinterpret_cast<float4*>(f + n0) = make_float4(S[0], S[1], S[2], S[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n0 + e < N) f[n0 + e] = S[e];
            }
        }
    }
    modes_publish(best, wl, best_key + b);
}

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

int posterior_parts(int64_t N)
{
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    return (int)(tiles < kTopkMaxParts ? tiles : kTopkMaxParts);
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

template <int kCtrl, int kRows, int kBanks>
__device__ __forceinline__ double sum_f64_dpp_step(double x)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, kCtrl, kRows, kBanks, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), kCtrl, kRows, kBanks, true);
    return x + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// sum over the 64 lanes in the order of wave_sum_dpp, in fp64; valid in lane 63
__device__ __forceinline__ double wave_sum_dpp_f64(double x)
{
    x = sum_f64_dpp_step<0x111, 0xF, 0xF>(x);  // row_shr:1
    x = sum_f64_dpp_step<0x112, 0xF, 0xF>(x);  // row_shr:2
    x = sum_f64_dpp_step<0x114, 0xF, 0xE>(x);  // row_shr:4
    x = sum_f64_dpp_step<0x118, 0xF, 0xC>(x);  // row_shr:8
    x = sum_f64_dpp_step<0x142, 0xA, 0xF>(x);  // row_bcast:15
    x = sum_f64_dpp_step<0x143, 0xC, 0xF>(x);  // row_bcast:31
    return x;
}

template <int kCtrl, int kRows>
__device__ __forceinline__ float max_f32_dpp_step(float x)
{
    const int xi = __builtin_bit_cast(int, x);
    const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, kCtrl, kRows, 0xF, false));
    return o > x ? o : x;
}

// the wave's largest value (no NaN among the inputs: they are finite scores or -inf), in every lane
__device__ __forceinline__ float wave_max_f32_dpp(float x)
{
    x = max_f32_dpp_step<0x111, 0xF>(x);
    x = max_f32_dpp_step<0x112, 0xF>(x);
    x = max_f32_dpp_step<0x114, 0xF>(x);
    x = max_f32_dpp_step<0x118, 0xF>(x);
    x = max_f32_dpp_step<0x142, 0xA>(x);
    x = max_f32_dpp_step<0x143, 0xC>(x);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
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

__device__ __forceinline__ int wave_max_int(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(x, off, 64);
        x = o > x ? o : x;
    }
    return x;
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
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
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

// out[b][j] = R[b][idx[b][j]] D[j], the product as compose_rotations_topk_kernel writes it; an index outside [0, N) composes row 0
__global__ __launch_bounds__(256) void compose_rotations_indexed_kernel(const long long* __restrict__ idx,
                                                                        const float* __restrict__ R, long r_batch_stride, long N,
                                                                        const float* __restrict__ D, long M, long total,
                                                                        float* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // b M + j
    if (i >= total) return;
    const long b = i / M;
    const long j = i - b * M;
    long n = (long)idx[i];
    n = (n < 0 || n >= N) ? 0 : n;  // -1 (a sample without a finite score) or a foreign list: stay in bounds
    const float* r = R + b * r_batch_stride + n * 9;
    const float* d = D + j * 9;
    float* o = out + i * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[a * 3 + c] = r[a * 3] * d[c] + r[a * 3 + 1] * d[3 + c] + r[a * 3 + 2] * d[6 + c];
}

// ---- SO(3) ascent step (ahv_so3_ascent_candidates_f32 / ahv_so3_ascent_select_f32) ----------------------
// One thread per seed (b, k); rotations.so3_ascent_candidates / so3_ascent_select state the same rules in torch.
// Direction: the Riemannian gradient in the body frame, w = vee(1/2 (R^T G - G^T R)); candidate slot 0 is R_cur bit for bit,
// slot l >= 1 is R_cur exp(ladder[l-1] theta [w / |w|]x) (Rodrigues, 1 - cos a as 2 sin^2(a / 2)); |w| = 0 or a non-finite w:
// every slot is R_cur.
__global__ __launch_bounds__(256) void so3_ascent_candidates_kernel(const float* __restrict__ R_cur, const float* __restrict__ grad_R,
                                                                    const float* __restrict__ theta, const float* __restrict__ ladder,
                                                                    int L, int seeds, float* __restrict__ R_cand)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= seeds) return;
    float R[9], G[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        R[j] = R_cur[(long)i * 9 + j];
        G[j] = grad_R[(long)i * 9 + j];
    }
    float A[9];   // R^T G
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = R[r] * G[c] + R[3 + r] * G[3 + c] + R[6 + r] * G[6 + c];
    const float wx = 0.5f * (A[7] - A[5]), wy = 0.5f * (A[2] - A[6]), wz = 0.5f * (A[3] - A[1]);
    const float nrm = sqrtf(wx * wx + wy * wy + wz * wz);
    const bool move = nrm > 0.0f && nrm < __builtin_inff();   // false for NaN
    const float inv = move ? 1.0f / nrm : 0.0f;
    const float nx = wx * inv, ny = wy * inv, nz = wz * inv;
    const float th = theta[i];
    float* out = R_cand + (long)i * (L + 1) * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) out[j] = R[j];
    for (int l = 1; l <= L; ++l) {
        float* o = out + l * 9;
        if (!move) {
#pragma unroll
            for (int j = 0; j < 9; ++j) o[j] = R[j];
            continue;
        }
        const float a = ladder[l - 1] * th;
        const float sn = sinf(a), sh = sinf(0.5f * a), c1 = 2.0f * sh * sh;
        // E = I + sin a K + (1 - cos a) (n n^T - I), K = [n]x
        const float E[9] = {1.0f + c1 * (nx * nx - 1.0f), c1 * nx * ny - sn * nz, c1 * nx * nz + sn * ny,
                            c1 * nx * ny + sn * nz, 1.0f + c1 * (ny * ny - 1.0f), c1 * ny * nz - sn * nx,
                            c1 * nx * nz - sn * ny, c1 * ny * nz + sn * nx, 1.0f + c1 * (nz * nz - 1.0f)};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[3 * r + c] = R[3 * r] * E[c] + R[3 * r + 1] * E[3 + c] + R[3 * r + 2] * E[6 + c];
    }
}

// A candidate replaces the incumbent only if its score is strictly greater (false for NaN), slots scanned in order: a seed's
// score never decreases, slot 0 (R_cur itself) wins a tie.  theta <- ladder[l-1] theta for the accepted slot, theta min(ladder)
// when slot 0 stayed.
__global__ __launch_bounds__(256) void so3_ascent_select_kernel(const float* __restrict__ R_cand, const float* __restrict__ cand_scores,
                                                                const float* __restrict__ ladder, int L, int seeds,
                                                                float* __restrict__ R_cur, float* __restrict__ score_cur,
                                                                float* __restrict__ theta)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= seeds) return;
    const float* sc = cand_scores + (long)i * (L + 1);
    float best = sc[0], lmin = ladder[0];
    int slot = 0;
    for (int l = 1; l <= L; ++l) {
        const float s = sc[l];
        if (s > best) {
            best = s;
            slot = l;
        }
        lmin = fminf(lmin, ladder[l - 1]);
    }
    const float* src = R_cand + ((long)i * (L + 1) + slot) * 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) R_cur[(long)i * 9 + j] = src[j];
    score_cur[i] = best;
    theta[i] = theta[i] * (slot ? ladder[slot - 1] : lmin);
}

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_argmax(const float* scores, int B, int64_t N, int64_t n_offset, int64_t* best_key,
                         int num_cu, hipStream_t stream)
{
    long bx = (N + 255) / 256;
    const long cap = num_cu * 4 / (B < num_cu ? B : num_cu) + 1;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, scores, B, (long)N,
                       (long)n_offset, reinterpret_cast<key_t*>(best_key));
    return hipGetLastError();
}

hipError_t launch_fill_keys(int64_t* best_key, int B, hipStream_t stream)
{
    hipLaunchKernelGGL(fill_keys_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, reinterpret_cast<key_t*>(best_key), B);
    return hipGetLastError();
}

// partial lists per sample of a top-K launch over N scores: a pure function of N (the workspace is sized by it)
int topk_parts(int64_t N)
{
    const int64_t tiles = (N + 3 + kTopkTile - 1) / kTopkTile;  // + 3: the row may start up to three floats past a 16-byte line
    return (int)(tiles < kTopkMaxParts ? tiles : kTopkMaxParts);
}

hipError_t launch_topk_merge(const int64_t* lists, int P, int B, int K, int64_t* keys, bool carry, hipStream_t stream)
{
    hipLaunchKernelGGL(topk_kernel<false>, dim3(1, (unsigned)B), dim3(kTopkThreads), 0, stream,
                       static_cast<const void*>(lists), B, (long)P, 0l, K, reinterpret_cast<key_t*>(keys), carry);
    return hipGetLastError();
}

hipError_t launch_topk(const float* scores, int B, int64_t N, int64_t n_offset, int K, int64_t* keys, int64_t* workspace,
                       bool carry, hipStream_t stream)
{
    const int parts = topk_parts(N);
    if (parts <= 1) {  // one tile: straight into the caller's list
        hipLaunchKernelGGL(topk_kernel<true>, dim3(1, (unsigned)B), dim3(kTopkThreads), 0, stream,
                           static_cast<const void*>(scores), B, (long)N, (long)n_offset, K, reinterpret_cast<key_t*>(keys),
                           carry);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(topk_kernel<true>, dim3((unsigned)parts, (unsigned)B), dim3(kTopkThreads), 0, stream,
                       static_cast<const void*>(scores), B, (long)N, (long)n_offset, K,
                       reinterpret_cast<key_t*>(workspace), false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_topk_merge(workspace, parts, B, K, keys, carry, stream);
}

hipError_t launch_select_topk(int64_t* keys, int K, const float* R, int64_t r_batch_stride, int64_t n_offset, int64_t N,
                              int B, float* R_out, float* scores_out, int64_t* idx_out, bool reset, hipStream_t stream)
{
    const long total = (long)B * K;
    hipLaunchKernelGGL(select_topk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<key_t*>(keys), K, R, (long)r_batch_stride, (long)n_offset, (long)N, B, R_out,
                       scores_out, reinterpret_cast<long*>(idx_out), reset);
    return hipGetLastError();
}

hipError_t launch_compose_rotations_topk(const int64_t* keys, int K, const float* R, int64_t r_batch_stride,
                                         int64_t n_offset, int64_t N, const float* D, int64_t N2, int B, float* out,
                                         hipStream_t stream)
{
    const long total = (long)B * K * N2;
    hipLaunchKernelGGL(compose_rotations_topk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const key_t*>(keys), K, R, (long)r_batch_stride, (long)n_offset, (long)N, D,
                       (long)N2, B, out);
    return hipGetLastError();
}

// hypotheses per sample of the alive state of ahv_topk_modes_f32: N rounded up to a lane's four
int64_t topk_modes_state_stride(int64_t N) { return (N + 3) & ~(int64_t)3; }

// K + 1 launches: the list filled EMPTY, round 0, rounds 1 .. K - 1 (each reads the entry the one before reduced)
hipError_t launch_topk_modes(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                             int K, float tau, int64_t* keys, int64_t* state, hipStream_t stream)
{
    hipError_t e = launch_fill_keys(keys, B * K, stream);
    if (e != hipSuccess) return e;
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    const long Ns = (long)topk_modes_state_stride(N);
    hipLaunchKernelGGL(topk_modes_kernel<true>, grid, dim3(kTopkThreads), 0, stream, scores, R, (long)r_batch_stride, (long)N,
                       Ns, (long)n_offset, K, 0, tau, reinterpret_cast<key_t*>(state), reinterpret_cast<key_t*>(keys));
    for (int j = 1; j < K; ++j)
        hipLaunchKernelGGL(topk_modes_kernel<false>, grid, dim3(kTopkThreads), 0, stream, scores, R, (long)r_batch_stride,
                           (long)N, Ns, (long)n_offset, K, j, tau, reinterpret_cast<key_t*>(state),
                           reinterpret_cast<key_t*>(keys));
    return hipGetLastError();
}

// ---- pose selection modulo a symmetry group ------------------------------------------------------------------
// launch_topk_modes with the rounds j >= 1 taken modulo the group (axis == nullptr: the finite part alone)
hipError_t launch_topk_modes_sym(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                                 int K, float tau, const float* S, int64_t s_batch_stride, int G, const float* axis,
                                 int64_t axis_batch_stride, int64_t* keys, int64_t* state, hipStream_t stream)
{
    hipError_t e = launch_fill_keys(keys, B * K, stream);
    if (e != hipSuccess) return e;
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    const long Ns = (long)topk_modes_state_stride(N);
    hipLaunchKernelGGL(topk_modes_kernel<true>, grid, dim3(kTopkThreads), 0, stream, scores, R, (long)r_batch_stride, (long)N,
                       Ns, (long)n_offset, K, 0, tau, reinterpret_cast<key_t*>(state), reinterpret_cast<key_t*>(keys));
    for (int j = 1; j < K; ++j) {
        if (axis)
            hipLaunchKernelGGL(topk_modes_sym_kernel<true>, grid, dim3(kTopkThreads), 0, stream, R, (long)r_batch_stride, (long)N, Ns,
                               (long)n_offset, K, j, tau, S, (long)s_batch_stride, G, axis, (long)axis_batch_stride,
                               reinterpret_cast<key_t*>(state), reinterpret_cast<key_t*>(keys));
        else
            hipLaunchKernelGGL(topk_modes_sym_kernel<false>, grid, dim3(kTopkThreads), 0, stream, R, (long)r_batch_stride, (long)N, Ns,
                               (long)n_offset, K, j, tau, S, (long)s_batch_stride, G, axis, (long)axis_batch_stride,
                               reinterpret_cast<key_t*>(state), reinterpret_cast<key_t*>(keys));
    }
    return hipGetLastError();
}

hipError_t launch_sym_fold(const float* R, int64_t r_batch_stride, int B, int64_t N, const float* S, int64_t s_batch_stride, int G,
                           const float* axis, int64_t axis_batch_stride, const float* anchors, int K, float tau, int64_t keep,
                           const float* V, float* R_out, float* V_out, int32_t* which, int32_t* elem, float* trace,
                           hipStream_t stream)
{
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    if (axis)
        hipLaunchKernelGGL(sym_fold_kernel<true>, grid, dim3(kTopkThreads), 0, stream, R, (long)r_batch_stride, (long)N, S,
                           (long)s_batch_stride, G, axis, (long)axis_batch_stride, anchors, K, tau, (long)keep, V, R_out, V_out, which,
                           elem, trace);
    else
        hipLaunchKernelGGL(sym_fold_kernel<false>, grid, dim3(kTopkThreads), 0, stream, R, (long)r_batch_stride, (long)N, S,
                           (long)s_batch_stride, G, axis, (long)axis_batch_stride, anchors, K, tau, (long)keep, V, R_out, V_out, which,
                           elem, trace);
    return hipGetLastError();
}

// ---- multi-view verification --------------------------------------------------------------------------------
hipError_t launch_view_rotations(const float* Q, int64_t q_batch_stride, const float* A, int B, int V, int64_t N, float* out,
                                 hipStream_t stream)
{
    const long total = (long)B * V * N;
    hipLaunchKernelGGL(view_rotations_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, Q,
                       (long)q_batch_stride, A, V, (long)N, total, out);
    return hipGetLastError();
}

// weights: V floats on the HOST, copied into the kernel arguments here (the launch itself reads no host memory)
hipError_t launch_fuse_views(const float* scores, const float* Q, int64_t q_batch_stride, const float* A, const float* weights,
                             int B, int V, int64_t N, int64_t n_offset, float tau, bool limit, float* fused, int64_t* best_key,
                             hipStream_t stream)
{
    ViewWeights w;
    for (int v = 0; v < kViewsMax; ++v) w.w[v] = v < V ? (weights ? weights[v] : 1.0f) : 0.0f;
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    hipLaunchKernelGGL(fuse_views_kernel, grid, dim3(kTopkThreads), 0, stream, scores, Q, (long)q_batch_stride, A, w, V, (long)N,
                       (long)n_offset, tau, limit, fused, reinterpret_cast<key_t*>(best_key));
    return hipGetLastError();
}

hipError_t launch_nearest_views(const float* anchor, const float* A, int B, int V, int K, int32_t* view_idx, float* A_sel,
                                hipStream_t stream)
{
    constexpr int per = kNearestThreads / kViewsMax;  // samples per workgroup
    hipLaunchKernelGGL(nearest_views_kernel, dim3((unsigned)((B + per - 1) / per)), dim3(kNearestThreads), 0, stream, anchor, A, B, V,
                       K, view_idx, A_sel);
    return hipGetLastError();
}

// L4: the row length in 16-byte units; grid (B K rows, up to 64 chunks of a row)
hipError_t launch_gather_views(const void* src, const int32_t* view_idx, int B, int V, int K, int64_t L4, void* dst, bool broadcast,
                               hipStream_t stream)
{
    const int64_t chunks = (L4 + kGatherThreads - 1) / kGatherThreads;
    const dim3 grid((unsigned)((int64_t)B * K), (unsigned)(chunks < 64 ? chunks : 64));
    hipLaunchKernelGGL(gather_views_kernel, grid, dim3(kGatherThreads), 0, stream, static_cast<const uint4*>(src), view_idx, V, K,
                       (long)L4, broadcast, static_cast<uint4*>(dst));
    return hipGetLastError();
}

// two launches: the per-tile counts into the workspace, then -- across the kernel boundary -- the slot map, the composed
// matrices, counts and the identity padding.  out == slot == nullptr: counts only (one summing workgroup per sample).
hipError_t launch_view_rotations_compact(const float* Q, int64_t q_batch_stride, const float* A, const float* weights, int B, int V,
                                         int64_t N, float tau, int64_t capacity, float* out, int32_t* slot, int64_t* counts,
                                         void* workspace, hipStream_t stream)
{
    ViewWeights w;
    for (int v = 0; v < kViewsMax; ++v) w.w[v] = v < V ? (weights ? weights[v] : 1.0f) : 0.0f;
    const int64_t tiles = view_compact_tiles(N);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    int* tc = static_cast<int*>(workspace);
    hipLaunchKernelGGL(view_compact_kernel<false>, grid, dim3(kTopkThreads), 0, stream, Q, (long)q_batch_stride, A, w, V, (long)N,
                       (long)tiles, tau, (long)capacity, tc, static_cast<float*>(nullptr), static_cast<int*>(nullptr),
                       static_cast<long long*>(nullptr));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(view_compact_kernel<true>, out ? grid : dim3(1u, (unsigned)B), dim3(kTopkThreads), 0, stream, Q,
                       (long)q_batch_stride, A, w, V, (long)N, (long)tiles, tau, (long)capacity, tc, out, slot,
                       reinterpret_cast<long long*>(counts));
    return hipGetLastError();
}

hipError_t launch_fuse_views_compact(const float* scores, const int32_t* slot, const float* weights, int B, int V, int64_t N,
                                     int64_t capacity, int64_t n_offset, float* fused, int64_t* best_key, hipStream_t stream)
{
    ViewWeights w;
    for (int v = 0; v < kViewsMax; ++v) w.w[v] = v < V ? (weights ? weights[v] : 1.0f) : 0.0f;
    const int64_t tiles = (N + kTopkTile - 1) / kTopkTile;
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
    hipLaunchKernelGGL(fuse_views_compact_kernel, grid, dim3(kTopkThreads), 0, stream, scores, slot, w, V, (long)N, (long)capacity,
                       (long)n_offset, fused, reinterpret_cast<key_t*>(best_key));
    return hipGetLastError();
}

// ---- pose posterior ---------------------------------------------------------------------------------------
hipError_t launch_posterior_merge(const void* states, int P, int B, int K, float beta, void* state, bool carry, hipStream_t stream)
{
    hipLaunchKernelGGL(posterior_merge_kernel, dim3((unsigned)B), dim3(64), 0, stream, static_cast<const char*>(states), P, B, K,
                       beta, static_cast<char*>(state), carry);
    return hipGetLastError();
}

// two launches: one partial state per workgroup into the workspace, then their merge into (or over) the caller's state
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

// ---- posterior resampling ---------------------------------------------------------------------------------
// three launches: a record per tile, the scan of the records, the draws (u: [B] on the device, or nullptr)
hipError_t launch_resample(const float* scores, int B, int64_t N, float beta, int64_t M, const float* u, int64_t* idx,
                           void* workspace, hipStream_t stream)
{
    const int64_t tiles = resample_tiles(N);
    const size_t stride = resample_stride(N);
    const dim3 grid((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)B);
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

hipError_t launch_compose_rotations_indexed(const int64_t* idx, const float* R, int64_t r_batch_stride, int64_t N, const float* D,
                                            int64_t M, int B, float* out, hipStream_t stream)
{
    const long total = (long)B * M;
    hipLaunchKernelGGL(compose_rotations_indexed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const long long*>(idx), R, (long)r_batch_stride, (long)N, D, (long)M, total, out);
    return hipGetLastError();
}

hipError_t launch_so3_ascent_candidates(const float* R_cur, const float* grad_R, const float* theta, const float* ladder, int L,
                                        int B, int K, float* R_cand, hipStream_t stream)
{
    const int seeds = B * K;
    if (seeds == 0) return hipSuccess;
    hipLaunchKernelGGL(so3_ascent_candidates_kernel, dim3((seeds + 255) / 256), dim3(256), 0, stream, R_cur, grad_R, theta,
                       ladder, L, seeds, R_cand);
    return hipGetLastError();
}

hipError_t launch_so3_ascent_select(const float* R_cand, const float* cand_scores, const float* ladder, int L, int B, int K,
                                    float* R_cur, float* score_cur, float* theta, hipStream_t stream)
{
    const int seeds = B * K;
    if (seeds == 0) return hipSuccess;
    hipLaunchKernelGGL(so3_ascent_select_kernel, dim3((seeds + 255) / 256), dim3(256), 0, stream, R_cand, cand_scores, ladder,
                       L, seeds, R_cur, score_cur, theta);
    return hipGetLastError();
}

}  // namespace ahv
