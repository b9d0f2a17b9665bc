// ahv_views.hip -- several posed reference views of one object: composing the per-view relative rotations, fusing the per-view
// scores into one score per hypothesis (whole and compact, under an angle limit), the nearest views of a pose and the gather of
// what belongs to them.  The kernels walk the tile rule of ahv_tile.h; view_compose_pinned, the product whose bytes the pose graph
// shares, is ahv_so3.h's.  Not here: the scorer the composed rotations go to
// (ahv_score.hip), the decode of the fused key (ahv_select.hip), the tracker that asks for the nearest views (ahv_track.hip).
#include "ahv_launch.h"
#include "ahv_so3.h"
#include "ahv_tile.h"

namespace ahv {

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

// weights: V floats on the host, or nullptr for 1 each; a slot past V holds 0 (an absent view)
inline ViewWeights make_view_weights(const float* weights, int V)
{
    ViewWeights w;
    for (int v = 0; v < kViewsMax; ++v) w.w[v] = v < V ? (weights ? weights[v] : 1.0f) : 0.0f;
    return w;
}

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

// ---- launchers ----------------------------------------------------------------------
hipError_t launch_view_rotations(const float* Q, int64_t q_batch_stride, const float* A, int B, int V, int64_t N, float* out,
                                 hipStream_t stream)
{
    const long total = (long)B * V * N;
    hipLaunchKernelGGL(view_rotations_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, Q,
                       (long)q_batch_stride, A, V, (long)N, total, out);
    return hipGetLastError();
}

hipError_t launch_fuse_views(const float* scores, const float* Q, int64_t q_batch_stride, const float* A, const float* weights,
                             int B, int V, int64_t N, int64_t n_offset, float tau, bool limit, float* fused, int64_t* best_key,
                             hipStream_t stream)
{
    const ViewWeights w = make_view_weights(weights, V);
    const dim3 grid = tile_grid(N, B);
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

hipError_t launch_gather_views(const void* src, const int32_t* view_idx, int B, int V, int K, int64_t L4, void* dst, bool broadcast,
                               hipStream_t stream)
{
    const int64_t chunks = (L4 + kGatherThreads - 1) / kGatherThreads;
    const dim3 grid((unsigned)((int64_t)B * K), (unsigned)(chunks < 64 ? chunks : 64));
    hipLaunchKernelGGL(gather_views_kernel, grid, dim3(kGatherThreads), 0, stream, static_cast<const uint4*>(src), view_idx, V, K,
                       (long)L4, broadcast, static_cast<uint4*>(dst));
    return hipGetLastError();
}

hipError_t launch_view_rotations_compact(const float* Q, int64_t q_batch_stride, const float* A, const float* weights, int B, int V,
                                         int64_t N, float tau, int64_t capacity, float* out, int32_t* slot, int64_t* counts,
                                         void* workspace, hipStream_t stream)
{
    const ViewWeights w = make_view_weights(weights, V);
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
    const ViewWeights w = make_view_weights(weights, V);
    const dim3 grid = tile_grid(N, B);
    hipLaunchKernelGGL(fuse_views_compact_kernel, grid, dim3(kTopkThreads), 0, stream, scores, slot, w, V, (long)N, (long)capacity,
                       (long)n_offset, fused, reinterpret_cast<key_t*>(best_key));
    return hipGetLastError();
}

}  // namespace ahv
