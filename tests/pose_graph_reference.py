"""numpy fp64 restatement of the joint pose inference kernels (``ahv_pose_graph_*_f32``, include/ahv.h), the planted graph both
test tiers solve, and the oracle-backed CPU backend of ``posegraph.PoseGraph``.  Plain module (like tests/views_reference.py).

    prim        Prim's maximum spanning tree from the root over the undirected graph: per step the edge with the largest finite
                score that joins a reached node to an unreached one, the lower edge index among equal scores
    propagate   A_j = P A_i entered from i, A_i = P^T A_j entered from j, in the order the tree was built
    candidates  slot 0 = A_k, slots 1..D = what each incident edge implies, the last F = fresh, the rest A_k exp([omega]x)
    edge_rotations  Q A_i^T (incoming) / A_j Q^T (outgoing)
    commit      A_k = Q[idx] where the key holds a finite score
"""
import itertools
import math

import numpy as np

from . import track_reference as tr
from . import track_views_reference as tvr
from . import views_reference as vr

OUTGOING = 1 << 30


def complete(V):
    return [(i, j) for i in range(V) for j in range(V) if i != j]


def incident(edges, V):
    """Per node the (edge id, outgoing) pairs in edge order."""
    inc = [[] for _ in range(V)]
    for e, (i, j) in enumerate(edges):
        inc[i].append((e, True))
        inc[j].append((e, False))
    return inc


def prim(score, edges, V, root=0):
    """score (E,) -> (parent_edge (V,), reached (V,), order [(edge, have, new), ...], gap): gap is the smallest difference
    between the best and the second-best DISTINCT candidate score of any step (inf when a step had one candidate or only exact
    ties): a test refuses a case whose gap is within rounding unless the ties are planted."""
    score = np.asarray(score, np.float64)
    parent = np.full(V, -1, np.int32)
    reached = np.zeros(V, np.int32)
    reached[root] = 1
    order, gap = [], np.inf
    for _ in range(V - 1):
        cand = [(e, i, j) for e, (i, j) in enumerate(edges) if reached[i] != reached[j] and np.isfinite(score[e])]
        if not cand:
            break
        best = max(cand, key=lambda c: (score[c[0]], -c[0]))
        others = [score[c[0]] for c in cand if score[c[0]] != score[best[0]]]
        if others:
            gap = min(gap, score[best[0]] - max(others))
        e, i, j = best
        have, new = (i, j) if reached[i] else (j, i)
        parent[new], reached[new] = e, 1
        order.append((e, have, new))
    return parent, reached, order, gap


def propagate(pair_R, edges, order, V, root=0):
    """-> (A (V,3,3) fp64, bound (V,3,3)): bound[v] = depth_v * sum |products| of the last product, the quantity the fp32
    error bound of the test scales (0 for the root and unreached nodes)."""
    P = np.asarray(pair_R, np.float64)
    A = np.tile(np.eye(3), (V, 1, 1))
    depth = np.zeros(V, np.int64)
    bound = np.zeros((V, 3, 3))
    for e, have, new in order:
        M = P[e] if edges[e][0] == have else P[e].T
        A[new] = M @ A[have]
        depth[new] = depth[have] + 1
        bound[new] = depth[new] * (np.abs(M) @ np.abs(A[have]))
    return A, bound


def tree_weight(score, tree):
    return float(sum(np.asarray(score, np.float64)[e] for e in tree))


def best_spanning_weight(score, edges, V, root=0):
    """Brute force (V <= 5): the largest total score of any spanning tree of the root's component over the finite edges."""
    score = np.asarray(score, np.float64)
    _, reached, order, _ = prim(score, edges, V, root)
    nodes = [v for v in range(V) if reached[v]]
    live = [e for e, (i, j) in enumerate(edges) if np.isfinite(score[e]) and reached[i] and reached[j]]
    best = -np.inf
    for pick in itertools.combinations(live, len(nodes) - 1):
        comp = {v: v for v in nodes}

        def find(v):
            while comp[v] != v:
                v = comp[v]
            return v
        ok = True
        for e in pick:
            a, b = find(edges[e][0]), find(edges[e][1])
            if a == b:
                ok = False
                break
            comp[a] = b
        if ok:
            best = max(best, tree_weight(score, pick))
    return best, tree_weight(score, [e for e, _, _ in order])


def neighbour(edges, entry):
    """(edge id, outgoing) -> the node at the other end."""
    e, out = entry
    return edges[e][1] if out else edges[e][0]


def candidates(A, pair_R, pair_score, edges, inc_k, k, omega, fresh=None):
    """One sample in fp64: A (V,3,3), omega (N,3) as applied in the noise slots -> Q (N,3,3)."""
    A, P = np.asarray(A, np.float64), np.asarray(pair_R, np.float64)
    N, D = len(omega), len(inc_k)
    Q = A[k][None] @ tr.exp_so3(np.asarray(omega, np.float64))
    Q[0] = A[k]
    for d, (e, out) in enumerate(inc_k):
        other = neighbour(edges, (e, out))
        Q[1 + d] = ((P[e].T if out else P[e]) @ A[other]) if np.isfinite(pair_score[e]) else A[k]
    if fresh is not None and len(fresh):
        Q[N - len(fresh):] = fresh
    return Q


def edge_rotations(Q, A, edges, inc_k):
    """Q (N,3,3), A (V,3,3) -> (D,N,3,3) fp64."""
    Q, A = np.asarray(Q, np.float64), np.asarray(A, np.float64)
    out = np.empty((len(inc_k),) + Q.shape)
    for d, (e, outgoing) in enumerate(inc_k):
        other = A[neighbour(edges, (e, outgoing))]
        out[d] = other[None] @ np.swapaxes(Q, -1, -2) if outgoing else Q @ other.T[None]
    return out


def commit(A, node_score, Q, keys, k):
    """In place on copies: A (B,V,3,3), node_score (B,V), Q (B,N,3,3), keys (B,) packed."""
    A, node_score = np.array(A), np.array(node_score)
    s, idx = vr.decode(np.asarray(keys))
    for b in range(len(A)):
        if keys[b] != vr.EMPTY and np.isfinite(s[b]) and 0 <= idx[b] < Q.shape[1]:
            A[b, k] = Q[b, idx[b]]
            node_score[b, k] = s[b]
    return A, node_score


def relative(A, edges):
    A = np.asarray(A, np.float64)
    return np.stack([A[..., j, :, :] @ np.swapaxes(A[..., i, :, :], -1, -2) for i, j in edges], axis=-3)


# ---- the planted graph ---------------------------------------------------------------------------------------------
# Complete graph on V nodes, every edge's source volume distinct, vol_tgt = rotate_volume(vol_src, A*_j A*_i^T): the maximum of
# every clean edge's score field is at the truth for any weights.  n_bad edges have their target replaced by an unrelated volume.
SIGMA_DEG = (6, 4, 3, 2, 1.5, 1, 0.75, 0.5)


def planted_truth(rotations, V, seed):
    R = rotations.haar_rotations_np(V, seed=4100 + seed).astype(np.float64)
    U, _, Vh = np.linalg.svd(R)
    return U @ Vh


def planted_bad(V, n_bad, seed):
    E = V * (V - 1)
    return sorted(np.random.default_rng(900 + seed).choice(E, size=n_bad, replace=False).tolist())


def planted_volumes(rotate, rotations, V, n_bad, seed):
    """``rotate(vol (1,16,8,8,8), R (3,3) fp64) -> (1,16,8,8,8)``.  -> (vol_src, vol_tgt (1,E,16,8,8,8) fp32, truth, bad)."""
    edges = complete(V)
    truth = planted_truth(rotations, V, seed)
    bad = planted_bad(V, n_bad, seed)
    rng = np.random.default_rng(7000 + seed)
    src = rng.standard_normal((len(edges), 16, 8, 8, 8)).astype(np.float32)
    tgt = np.empty_like(src)
    for e, (i, j) in enumerate(edges):
        tgt[e] = (rng.standard_normal((16, 8, 8, 8)).astype(np.float32) if e in bad
                  else rotate(src[e][None], truth[j] @ truth[i].T)[0])
    return src[None], tgt[None], truth, bad


def planted_figures(res_A, res_pair_R, parent_edge, truth, bad, V):
    """-> dict: joint max / median over ALL ordered pairs, pairwise clean median / max, the bad edges' pairwise errors, tree uses
    a bad edge.  Errors in degrees, fp64."""
    edges = complete(V)
    gt = relative(truth, edges)
    joint = tr.geodesic_deg(relative(np.asarray(res_A, np.float64), edges), gt)
    pair = tr.geodesic_deg(np.asarray(res_pair_R, np.float64), gt)
    clean = [e for e in range(len(edges)) if e not in bad]
    return dict(joint_max=float(joint.max()), joint_median=float(np.median(joint)), pair_clean_median=float(np.median(pair[clean])),
                pair_clean_max=float(pair[clean].max()), pair_bad=[float(pair[e]) for e in bad],
                bad_in_tree=sorted(set(int(e) for e in np.asarray(parent_edge).reshape(-1)) & set(bad)))


# ---- oracle-backed CPU backend of posegraph.PoseGraph -------------------------------------------------------------------
def make_backend(ahv, oracle):
    """``track_views_reference.make_backend`` (verify_pair, select_rotation, track_advance, gather_views) plus the four graph
    ops: the tree, the candidates, the edge rotations and the commit are this module's rounded to fp32, the scores the CPU
    oracle's per incident edge, the fusion ``views_reference.fuse``; numpy draws the noise, seeded by (seed, counter, sweep, k).
    Test infrastructure: the product backend is HIP."""
    import torch

    base = tvr.make_backend(ahv, oracle)

    class PoseGraphOracleBackend(type(base)):
        def pose_graph_init(self, pair_R, pair_score, topology, out=None):
            assert out is not None
            V, edges = topology.n_views, topology.edges
            for b in range(pair_R.shape[0]):
                parent, reached, order, _ = prim(pair_score[b].numpy(), edges, V, topology.root)
                A, _ = propagate(pair_R[b].numpy(), edges, order, V, topology.root)
                out[0][b] = torch.from_numpy(A.astype(np.float32))
                out[1][b] = torch.from_numpy(parent)
                out[2][b] = torch.from_numpy(reached)
            self.calls.append("pose_graph_init")
            return ahv.ops.PoseGraphInit(*out)

        def pose_graph_propose(self, A, pair_R, pair_score, topology, k, n, sigma_deg, sweep=0, seed=0, counter=None, n_fresh=0,
                               out=None):
            assert out is not None and k != topology.root
            Q, Rrel = out
            B = A.shape[0]
            t = 0 if counter is None else int(counter[0])
            rs = np.random.RandomState([seed & 0xFFFFFFFF, t, sweep, k])
            for b in range(B):
                omega = math.radians(sigma_deg) * rs.standard_normal((n, 3))
                fresh = ahv.rotations.haar_rotations_np(n_fresh, seed=int(rs.randint(1 << 30))) if n_fresh else None
                q = candidates(A[b].numpy(), pair_R[b].numpy(), pair_score[b].numpy(), topology.edges, topology.incident[k], k, omega,
                               fresh).astype(np.float32)
                q[0] = A[b, k].numpy()
                Q[b] = torch.from_numpy(q)
                Rrel[b] = torch.from_numpy(edge_rotations(q, A[b].numpy(), topology.edges, topology.incident[k]).astype(np.float32))
            self.calls.append("pose_graph_propose:%d" % k)
            return Q, Rrel

        def pose_graph_score(self, vol_src, vol_tgt, Rrel, W1, W2, b2, weights=None, workspace=None, scores_out=None,
                             best_key=None, split_f16=None):
            B, D, N = Rrel.shape[:3]
            w = (W1.numpy(), W2.numpy(), b2.numpy())
            s = np.zeros((B, D, N), np.float32)
            for b in range(B):
                for d in range(D):
                    if weights is None or weights[d] > 0:
                        s[b, d] = oracle.score_hypotheses(vol_src[b, d][None].numpy(), vol_tgt[b, d][None].numpy(), Rrel[b, d].numpy(), *w)[0][0]
            S, _, _, _ = vr.fuse(s, None, None, weights, None)
            S = S.astype(np.float32)
            scores_out.copy_(torch.from_numpy(S))
            best_key.copy_(torch.from_numpy(vr.best_keys(S)))
            self.last_edge_scores = s
            self.calls.append("pose_graph_score")
            return scores_out, best_key

        def pose_graph_commit(self, key, Q, A, node_score, k):
            newA, news = commit(A.numpy(), node_score.numpy(), Q.numpy(), key.numpy(), k)
            A.copy_(torch.from_numpy(newA))
            node_score.copy_(torch.from_numpy(news))
            self.calls.append("pose_graph_commit:%d" % k)
            return A, node_score

    return PoseGraphOracleBackend()
