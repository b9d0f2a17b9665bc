// ahv_graph.hip -- joint pose inference over an unposed image set (ahv_pose_graph_*_f32, include/ahv.h): V images, E directed
// edges (i -> j) that each carry an independent pairwise estimate pair_R[e] of A_j A_i^T with its score, and absolute rotations
// A_v wanted for all images at once.  Three small kernels around the unchanged scoring launch of ahv_score.hip:
//   pose_graph_init_kernel     a maximum spanning tree of the most confident pairs (Prim from the root) and the absolute
//                              rotations the tree implies
//   pose_graph_propose_kernel  the candidates Q_n of one node's rotation and, per incident edge, the relative rotation the
//                              scorer sees for each of them
//   pose_graph_commit_kernel   the winner of the fused row written back into A
// The topology is static: the edge list and a node's incident list are int32 arrays the caller uploaded once.  The kernels
// validate every index they read from them (a foreign list stays in bounds; the host refuses it before).  Plain launches: no
// atomics, no workgroup waits on another one, every sum in one stated order.
#include "ahv_device.h"
#include "ahv_launch.h"
#include "ahv_so3.h"

namespace ahv {

constexpr int kGraphNodesMax = 16;             // AHV_GRAPH_MAX_NODES
constexpr int kGraphOutgoing = 1 << 30;        // AHV_GRAPH_EDGE_OUTGOING: the direction bit of an incident-list entry
constexpr unsigned kGraphTag = 0x504752u;      // third counter word of a candidate's noise block (low 24 bits; node k above)
constexpr unsigned long long kGraphFreshSeed = 0x9E3779B97F4A7C15ull;  // as the tracker's fresh slots: seed ^ this

__device__ __forceinline__ bool graph_finite(float x) { return fabsf(x) < __builtin_inff(); }  // false for NaN

// o = P x (transposed = false) or P^T x (true), 3x3 row-major: entry (a, c) = fma(p2, x[2][c], fma(p1, x[1][c], p0 x[0][c]))
// with p_m = P[a][m] or P[m][a] -- the one product rule of the tree propagation and of the neighbour proposals.
__device__ __forceinline__ float graph_product_entry(const float* __restrict__ P, bool transposed, const float* x, int a, int c)
{
#pragma clang fp contract(off)
    const float p0 = transposed ? P[a] : P[a * 3], p1 = transposed ? P[3 + a] : P[a * 3 + 1], p2 = transposed ? P[6 + a] : P[a * 3 + 2];
    return fmaf(p2, x[6 + c], fmaf(p1, x[3 + c], p0 * x[c]));
}

// ---------------------------------------------------------------------------------
// The tree: one wave per sample.  The set of reached nodes is a 16-bit mask every lane holds (uniform); per step lane l packs
// the key (score, e) of every edge e = l, l + 64, ... that joins a reached node to an unreached one -- pack_key orders by score
// descending and edge index ascending, the rule of topk -- the wave takes the maximum by shuffles, and lanes 0..8 write
// the nine entries of the new node's rotation into LDS.  V - 1 steps of ceil(E / 64) edge reads: latency-bound by the
// dependent chain (score load -> wave max -> edge load -> rotation load -> product).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pose_graph_init_kernel(const float* __restrict__ pair_R, const float* __restrict__ pair_score,
                                                             const int* __restrict__ edges, int V, int E, int root,
                                                             float* __restrict__ A, int* __restrict__ parent_edge,
                                                             int* __restrict__ reached)
{
    __shared__ float As[kGraphNodesMax][9];
    __shared__ int parent[kGraphNodesMax];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const float* Pb = pair_R + b * E * 9;
    const float* sb = pair_score + b * E;
    if (lane < kGraphNodesMax) parent[lane] = -1;
    if (lane < 9) As[root][lane] = (lane == 0 || lane == 4 || lane == 8) ? 1.0f : 0.0f;
    __syncthreads();
    unsigned in_tree = 1u << root;
    for (int step = 1; step < V; ++step) {
        key_t best = kKeyEmpty;
        for (int e = lane; e < E; e += 64) {
            const int i = edges[2 * e], j = edges[2 * e + 1];
            if (i < 0 || i >= V || j < 0 || j >= V) continue;
            const bool crosses = (((in_tree >> i) ^ (in_tree >> j)) & 1u) != 0;
            const float s = sb[e];
            if (!crosses || !graph_finite(s)) continue;
            const key_t k = pack_key(s, (unsigned)e);
            best = k > best ? k : best;
        }
        best = wave_max_key(best);
        if (best == kKeyEmpty) break;  // uniform: the rest of the graph is not connected to the root
        const int e = (int)key_index(best);
        const int i = edges[2 * e], j = edges[2 * e + 1];
        const bool from_i = ((in_tree >> i) & 1u) != 0;  // entered from i: A_j = P A_i; from j: A_i = P^T A_j
        const int have = from_i ? i : j, fresh = from_i ? j : i;
        if (lane < 9) As[fresh][lane] = graph_product_entry(Pb + (long)e * 9, !from_i, As[have], lane / 3, lane % 3);
        if (lane == 0) parent[fresh] = e;
        in_tree |= 1u << fresh;
        __syncthreads();
    }
    for (int t = lane; t < V * 9; t += 64) {
        const int v = t / 9, c = t - v * 9;
        const bool in = ((in_tree >> v) & 1u) != 0;
        A[(b * V + v) * 9 + c] = in ? As[v][c] : ((c == 0 || c == 4 || c == 8) ? 1.0f : 0.0f);
    }
    if (lane < V) {
        parent_edge[b * V + lane] = parent[lane];
        reached[b * V + lane] = (int)((in_tree >> lane) & 1u);
    }
}

// ---------------------------------------------------------------------------------
// The candidates of node k and what each incident edge makes of them: one thread per (b, n).  Slot classes, in this precedence:
//   current    n == 0: A[b][k], bit for bit
//   neighbour  1 <= n <= D: what incident edge d = n - 1 implies, P A_i (incoming, i -> k) or P^T A_j (outgoing, k -> j) under
//              graph_product_entry; a non-finite pair_score: A[b][k], bit for bit
//   fresh      n >= N - n_fresh: a rotation of the Haar stream of seed ^ kGraphFreshSeed
//   else       A[b][k] exp([sigma z]x) composed as unit quaternions and normalised (compose_rotation_vector, as the tracker)
// The thread then walks the incident list: Rrel[b][d][n] = Q_n A_i^T (incoming; view_compose_pinned: the bytes of
// view_rotations_kernel) or A_j Q_n^T (outgoing; the same operations with A_j in the place of Q_n and Q_n in that of A_i).
// A[b][.] and the list are uniform over a workgroup (scalar loads); a thread writes 36 (D + 1) bytes.  Bound by launch latency and
// the write of B D N matrices: 258 KB at D = 14, N = 512.
// ---------------------------------------------------------------------------------
struct GraphNeighbour {
    int e, node;  // both validated: inside [0, E) and [0, V)
    bool outgoing;
};

__device__ __forceinline__ GraphNeighbour graph_neighbour(const int* __restrict__ edges, const int* __restrict__ incident, int d,
                                                          int V, int E)
{
    const int w = incident[d];
    GraphNeighbour g;
    g.outgoing = (w & kGraphOutgoing) != 0;
    const int e = w & (kGraphOutgoing - 1);
    g.e = (e < 0 || e >= E) ? 0 : e;
    const int node = edges[2 * g.e + (g.outgoing ? 1 : 0)];  // the other end: the target of an outgoing edge, else the source
    g.node = (node < 0 || node >= V) ? 0 : node;
    return g;
}

__global__ __launch_bounds__(256) void pose_graph_propose_kernel(const float* __restrict__ A, const float* __restrict__ pair_R,
                                                                 const float* __restrict__ pair_score, const int* __restrict__ edges,
                                                                 const int* __restrict__ incident, int V, int E, int k, int D, long N,
                                                                 long n_fresh, unsigned long long seed,
                                                                 const long long* __restrict__ counter, int sweep, float sigma,
                                                                 float* __restrict__ Q, float* __restrict__ Rrel)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const long b = blockIdx.y;
    const float* Ab = A + b * V * 9;
    const float* ak = Ab + k * 9;
    const float cur[9] = {ak[0], ak[1], ak[2], ak[3], ak[4], ak[5], ak[6], ak[7], ak[8]};
    float q[9];
    if (n >= 1 && n <= D) {
        const GraphNeighbour g = graph_neighbour(edges, incident, (int)n - 1, V, E);
        if (graph_finite(pair_score[b * E + g.e])) {
            const float* P = pair_R + (b * E + g.e) * 9;
            const float* x = Ab + g.node * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) q[t] = graph_product_entry(P, g.outgoing, x, t / 3, t % 3);
        } else {
#pragma unroll
            for (int t = 0; t < 9; ++t) q[t] = cur[t];
        }
    } else if (n == 0) {
#pragma unroll
        for (int t = 0; t < 9; ++t) q[t] = cur[t];
    } else {
        const unsigned long long t = counter ? (unsigned long long)*counter : 0ull;
        if (n >= N - n_fresh) {
            const unsigned long long ctr =
                ((((t * 256ull + (unsigned long long)sweep) * 65536ull + (unsigned long long)b) * 16ull + (unsigned long long)k)
                 * (unsigned long long)N) + (unsigned long long)n;
            haar_rotation(seed ^ kGraphFreshSeed, ctr, q);
        } else {
            unsigned c[4] = {(unsigned)n, (unsigned)b | ((unsigned)sweep << 16) | ((unsigned)(t >> 32) << 24),
                             kGraphTag | ((unsigned)k << 24), (unsigned)t};
            philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
            float z0, z1, z2, z3;
            box_muller4(c, z0, z1, z2, z3);
            compose_rotation_vector(cur, sigma * z0, sigma * z1, sigma * z2, q);
        }
    }
    float* qo = Q + (b * N + n) * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) qo[t] = q[t];
    for (int d = 0; d < D; ++d) {
        const GraphNeighbour g = graph_neighbour(edges, incident, d, V, E);
        const float* x = Ab + g.node * 9;
        float o[9];
        if (g.outgoing) {
            const float aj[9] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8]};
            view_compose_pinned(aj, q, o);
        } else {
            view_compose_pinned(q, x, o);
        }
        float* ro = Rrel + ((b * D + d) * N + n) * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) ro[t] = o[t];
    }
}

// One thread per sample: the packed key of the fused row -> A[b][k] = Q[b][idx] (bit copy) and node_score[b][k].  A key that is
// EMPTY, decodes outside [0, N) or holds a non-finite score leaves both untouched.
__global__ __launch_bounds__(256) void pose_graph_commit_kernel(const key_t* __restrict__ key, const float* __restrict__ Q, int B,
                                                                int V, int k, long N, float* __restrict__ A,
                                                                float* __restrict__ node_score)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const key_t kk = key[b];
    if (kk == kKeyEmpty) return;
    const long idx = key_index(kk);
    const float s = key_score(kk);
    if (idx < 0 || idx >= N || !graph_finite(s)) return;
    const float* q = Q + ((long)b * N + idx) * 9;
    float* a = A + ((long)b * V + k) * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) a[t] = q[t];
    node_score[(long)b * V + k] = s;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
hipError_t launch_pose_graph_init(const float* pair_R, const float* pair_score, const int32_t* edges, int B, int V, int E, int root,
                                  float* A, int32_t* parent_edge, int32_t* reached, hipStream_t stream)
{
    hipLaunchKernelGGL(pose_graph_init_kernel, dim3((unsigned)B), dim3(64), 0, stream, pair_R, pair_score, edges, V, E, root, A,
                       parent_edge, reached);
    return hipGetLastError();
}

hipError_t launch_pose_graph_propose(const float* A, const float* pair_R, const float* pair_score, const int32_t* edges,
                                     const int32_t* incident, int B, int V, int E, int k, int D, int64_t N, int64_t n_fresh,
                                     uint64_t seed, const int64_t* counter, int sweep, float sigma, float* Q, float* Rrel,
                                     hipStream_t stream)
{
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(pose_graph_propose_kernel, grid, dim3(256), 0, stream, A, pair_R, pair_score, edges, incident, V, E, k, D,
                       (long)N, (long)n_fresh, (unsigned long long)seed, reinterpret_cast<const long long*>(counter), sweep, sigma, Q,
                       Rrel);
    return hipGetLastError();
}

hipError_t launch_pose_graph_commit(const int64_t* key, const float* Q, int B, int V, int k, int64_t N, float* A, float* node_score,
                                    hipStream_t stream)
{
    hipLaunchKernelGGL(pose_graph_commit_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const key_t*>(key), Q, B, V, k, (long)N, A, node_score);
    return hipGetLastError();
}

}  // namespace ahv
