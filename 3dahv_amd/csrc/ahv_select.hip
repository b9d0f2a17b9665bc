// ahv_select.hip -- pose selection from scores that exist: packed keys (arg-max, fill), K-best lists (top-K, merge, decode +
// gather, the compose kernels), distinct modes -- plain and modulo a symmetry group, with the fold into a fundamental domain
// (ahv_sym.h) -- and the SO(3) ascent step.  These kernels read scores, keys and rotation matrices only: no volume, no MFMA.
// Not here: the multi-view kernels (ahv_views.hip), the pose posterior and the draws from it (ahv_posterior.hip) -- they share
// the tile rule of the modes kernels (ahv_tile.h) and nothing of the list machinery --, and unpack_best_kernel, the decode
// without a gather, which sits with the scorer in ahv_score.hip.
#include "ahv_launch.h"
#include "ahv_so3.h"
#include "ahv_sym.h"
#include "ahv_tile.h"

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
// (kTopkThreads, kTopkPerLane and kTopkTile are ahv_tile.h's: the modes, view and posterior kernels walk the same tiles)
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

int64_t topk_modes_state_stride(int64_t N) { return (N + 3) & ~(int64_t)3; }

hipError_t launch_topk_modes(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                             int K, float tau, int64_t* keys, int64_t* state, hipStream_t stream)
{
    hipError_t e = launch_fill_keys(keys, B * K, stream);
    if (e != hipSuccess) return e;
    const dim3 grid = tile_grid(N, B);
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
hipError_t launch_topk_modes_sym(const float* scores, const float* R, int64_t r_batch_stride, int B, int64_t N, int64_t n_offset,
                                 int K, float tau, const float* S, int64_t s_batch_stride, int G, const float* axis,
                                 int64_t axis_batch_stride, int64_t* keys, int64_t* state, hipStream_t stream)
{
    hipError_t e = launch_fill_keys(keys, B * K, stream);
    if (e != hipSuccess) return e;
    const dim3 grid = tile_grid(N, B);
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
    const dim3 grid = tile_grid(N, B);
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
