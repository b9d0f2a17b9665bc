"""Joint pose inference over an unposed image set, on the device: ``ahv_pose_graph_init_f32`` / ``ahv_pose_graph_propose_f32`` /
``ahv_pose_graph_commit_f32`` against the numpy fp64 reference (tests/pose_graph_reference.py), one node update end to end
against the CPU oracle, the monotonicity of the ascent, and the planted graph with ``posegraph.PoseGraph`` eager and captured.

Bounds (u = 2^-24, the unit roundoff of fp32):
  one 3x3 product entry  fma(p2, x2, fma(p1, x1, p0 x0)) is three rounded operations: |error| <= gamma_3 sum|p x| < 4 u sum|p x|
                         (gamma_3 = 3u / (1 - 3u)).  That is the bound of a neighbour proposal and of an outgoing edge rotation.
  tree propagation       a node at depth d is d such products in a row; the factor of each is a rotation (rows of norm 1, so the
                         error a factor carries forward is not amplified beyond sum|p x| of the next product, which is <= 3):
                         |error| <= 4 * d * 3 u * sum|products| per element, sum|products| taken at the node's own (last) product.

Figures measured on the MI355X (this file prints them; README and DESIGN 4.2 quote them):
  planted graph, V = 5, 3 bad edges, seeds 0 / 1 / 2: joint max 0.267 / 0.248 / 0.523 degrees against a pairwise clean median of
  9.120 / 8.673 / 9.461; tree max 10.7 / 8.6 / 13.2; clean scores >= 0.745, bad <= 0.511
  one node update (V = 3, N = 64, B = 2): fused row within 2.8e-07 relative of the oracle's scores averaged in fp64
  noise at sigma = 3 degrees: mean squared angle 26.93 deg^2 over 4 096 slots (3 sigma^2 = 27)
"""

import numpy as np
import pytest
import torch

from . import pose_graph_reference as pgr
from . import track_reference as tr
from . import views_reference as vr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
VOL = (16, 8, 8, 8)
U = 2.0 ** -24
FRESH_XOR = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


@pytest.fixture(scope="module")
def head(dev):
    h = load_golden("score_n128")
    return tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _bytes_equal(a, b):
    return torch.equal(_bits(a), _bits(b))


def _pairs(ahv, B, E, seed):
    """pair_R (B,E,3,3) Haar fp32 and well-separated scores (B,E): a permutation of a grid of step 1e-2, jittered by < 1e-3."""
    P = ahv.rotations.haar_rotations_np(B * E, seed=seed).reshape(B, E, 3, 3)
    rng = np.random.default_rng(seed)
    s = np.stack([rng.permutation(E) * 1e-2 + rng.uniform(0, 1e-3, E) - 0.3 for _ in range(B)]).astype(np.float32)
    return P, s


# ---- 1. pose_graph_init ----------------------------------------------------------------------------------------------------
def _check_init(ops, dev, P, s, edges, V, root, planted_ties=False):
    top = ops.PoseGraphTopology(V, edges, root, device=dev)
    got = ops.pose_graph_init(_t(P).to(dev), _t(s).to(dev), top)
    A = got.A.cpu().double().numpy()
    for b in range(len(P)):
        parent, reached, order, gap = pgr.prim(s[b], edges, V, root)
        assert gap > 1e-4, "the case is too close to call: top two candidates %.3e apart" % gap
        assert planted_ties or len(set(s[b][np.isfinite(s[b])].tolist())) == np.isfinite(s[b]).sum()
        assert np.array_equal(got.parent_edge[b].cpu().numpy(), parent), (V, b)
        assert np.array_equal(got.reached[b].cpu().numpy(), reached), (V, b)
        ref, bound = pgr.propagate(P[b], edges, order, V, root)
        err = np.abs(A[b] - ref)
        assert (err <= 4.0 * 3.0 * U * bound).all(), (V, b, float(err.max()))
        for v in range(V):
            if v == root or not reached[v]:
                assert np.array_equal(got.A[b, v].cpu().numpy(), np.eye(3, dtype=np.float32))
    return got


@pytest.mark.parametrize("B", [1, 3])
def test_init_matches_the_reference_tree(ahv, ops, dev, B):
    for V in (2, 3, 5, 9):
        edges = pgr.complete(V)
        P, s = _pairs(ahv, B, len(edges), seed=40 + V)
        _check_init(ops, dev, P, s, edges, V, root=V // 2)
    # a ring of 16 nodes, one direction only: the tree is the ring minus its weakest edge, depth up to 15
    ring = [(v, (v + 1) % 16) for v in range(16)]
    P, s = _pairs(ahv, B, 16, seed=77)
    _check_init(ops, dev, P, s, ring, 16, root=0)
    # an isolated node (3) and a component the root does not reach (4 - 5)
    edges = [(0, 1), (2, 1), (0, 2), (4, 5), (5, 4)]
    P, s = _pairs(ahv, B, len(edges), seed=78)
    got = _check_init(ops, dev, P, s, edges, 6, root=0)
    assert got.reached.cpu().tolist() == [[1, 1, 1, 0, 0, 0]] * B and (got.parent_edge[:, 3:] == -1).all()


@pytest.mark.parametrize("B", [1, 3])
def test_init_non_finite_scores_and_exact_ties(ahv, ops, dev, B):
    V = 5
    edges = pgr.complete(V)
    P, s = _pairs(ahv, B, len(edges), seed=91)
    best = np.argsort(-s, axis=1)
    for b in range(B):
        s[b, best[b, 0]] = np.nan                 # the strongest edges are absent, whatever their kind
        s[b, best[b, 1]] = np.inf
        s[b, best[b, 2]] = -np.inf
        s[b, best[b, 4]] = s[b, best[b, 3]]       # an exact tie at the top of what is left: the lower edge index wins
        s[b, best[b, 5]], s[b, best[b, 6]] = 0.0, -0.0   # and a +0 / -0 pair (every other score is negative): equal
    _check_init(ops, dev, P, s, edges, V, root=0, planted_ties=True)
    # every edge tied: the tree is the reference's, by index alone
    _check_init(ops, dev, P, np.full_like(s, 0.25), edges, V, root=3, planted_ties=True)
    # nothing finite: every node keeps the identity
    got = _check_init(ops, dev, P, np.full_like(s, np.nan), edges, V, root=1, planted_ties=True)
    assert (got.reached.sum(dim=1) == 1).all()


# ---- 2. pose_graph_propose -----------------------------------------------------------------------------------------------
GRAPHS = {1: (2, [(0, 1)], 1), 2: (3, [(0, 1), (1, 2)], 1), 8: (5, None, 2), 16: (9, None, 4)}   # D -> (V, edges, k)


def _propose_case(ahv, ops, dev, D, B, N, n_fresh, seed=11, sweep=3, t=5):
    V, edges, k = GRAPHS[D]
    top = ops.PoseGraphTopology(V, edges, 0, device=dev)
    assert top.degree[k] == D
    E = top.n_edges
    P, s = _pairs(ahv, B, E, seed=200 + D)
    inc = top.incident[k]
    dead = inc[len(inc) // 2][0]
    s[:, dead] = np.nan                                                        # one incident edge proposes the fallback
    A = ahv.rotations.haar_rotations_np(B * V, seed=300 + D).reshape(B, V, 3, 3)
    counter = torch.tensor([t], dtype=torch.int64, device=dev)
    Ad, Pd, sd = _t(A).to(dev), _t(P).to(dev), _t(s).to(dev)
    Q, Rrel = ops.pose_graph_propose(Ad, Pd, sd, top, k, N, 3.0, sweep=sweep, seed=seed, counter=counter, n_fresh=n_fresh)
    return top, k, A, P, s, Ad, Q, Rrel, dead


@pytest.mark.parametrize("D", [1, 2, 8, 16])
def test_propose_slots_and_edge_rotations(ahv, ops, dev, D):
    seed, sweep, t = 11, 3, 5
    for B in (1, 3):
        for N in sorted({1 + D, 33, 64, 65, 257}):
            for n_fresh in sorted({0, min(4, N - 1 - D)}):
                top, k, A, P, s, Ad, Q, Rrel, dead = _propose_case(ahv, ops, dev, D, B, N, n_fresh, seed, sweep, t)
                assert tuple(Q.shape) == (B, N, 3, 3) and tuple(Rrel.shape) == (B, D, N, 3, 3)
                Qh = Q.cpu()
                assert _bytes_equal(Qh[:, 0], _t(A[:, k]))                                        # slot 0: bit for bit
                Qd = Qh.double().numpy()
                for d, (e, out) in enumerate(top.incident[k]):
                    other = pgr.neighbour(top.edges, (e, out))
                    if e == dead:
                        assert _bytes_equal(Qh[:, 1 + d], _t(A[:, k]))                            # the fallback: bit for bit
                    else:
                        M = np.swapaxes(P[:, e], -1, -2) if out else P[:, e]
                        want = M.astype(np.float64) @ A[:, other].astype(np.float64)
                        tol = 4.0 * U * (np.abs(M).astype(np.float64) @ np.abs(A[:, other]).astype(np.float64))
                        assert (np.abs(Qd[:, 1 + d] - want) <= tol).all(), (D, B, N, d)
                    # the edge rotations of EVERY slot
                    if out:
                        Aj = A[:, other].astype(np.float64)
                        want = Aj[:, None] @ np.swapaxes(Qd, -1, -2)
                        tol = 4.0 * U * (np.abs(Aj)[:, None] @ np.abs(np.swapaxes(Qd, -1, -2)))
                        assert (np.abs(Rrel[:, d].cpu().double().numpy() - want) <= tol).all(), (D, B, N, d)
                    else:
                        same = ops.view_rotations(Q, Ad[:, other:other + 1].contiguous())
                        assert _bytes_equal(Rrel[:, d], same[:, 0]), (D, B, N, d)                   # the bytes of view_rotations
                if n_fresh:
                    for b in range(B):
                        ctr = ((((t * 256 + sweep) * 65536 + b) * 16 + k) * N + (N - n_fresh)) & (2**64 - 1)
                        want = ops.random_rotations(n_fresh, seed=seed ^ FRESH_XOR, offset=ctr, device=dev)
                        assert _bytes_equal(Q[b, N - n_fresh:], want), (D, B, N, b)
                # the noise slots sit on SO(3) as well as the sampler's own output does
                lo, hi = 1 + D, N - n_fresh
                if hi - lo >= 200:      # (the bar of tests/test_gpu_track.py's drift test: 4 x the sampler's own defect at that size)
                    defect = lambda R: float((R.double().transpose(-1, -2) @ R.double() - torch.eye(3, dtype=torch.float64)).abs().max())
                    base = defect(ops.random_rotations(B * (hi - lo), seed=3, device=dev).cpu())
                    assert defect(Qh[:, lo:hi]) <= 4.0 * base, (D, B, N)


def test_propose_noise_is_a_function_of_its_slot_alone(ahv, ops, dev):
    V, k, N = 5, 2, 64
    top5 = ops.PoseGraphTopology(V, None, 0, device=dev)
    P, s = _pairs(ahv, 3, top5.n_edges, seed=21)
    A = ahv.rotations.haar_rotations_np(3 * V, seed=22).reshape(3, V, 3, 3)
    Ad, Pd, sd = _t(A).to(dev), _t(P).to(dev), _t(s).to(dev)

    def run(inputs=(Ad, Pd, sd, top5), k=k, n=N, sweep=1, seed=9, t=4):
        counter = torch.tensor([t], dtype=torch.int64, device=dev)
        return ops.pose_graph_propose(*inputs, k, n, 3.0, sweep=sweep, seed=seed, counter=counter)[0]

    Q = run()
    first = 1 + top5.degree[k]
    assert _bytes_equal(Q, run())                                                                  # reproducible
    # one sample alone, a longer set, and a smaller graph around the same node rotation: the same noise slots
    alone = run(inputs=(Ad[:1].contiguous(), Pd[:1].contiguous(), sd[:1].contiguous(), top5))
    assert _bytes_equal(alone[0], Q[0])
    assert _bytes_equal(run(n=65)[:, first:N], Q[:, first:])
    top3 = ops.PoseGraphTopology(3, None, 0, device=dev)
    small = run(inputs=(Ad[:, :3].contiguous(), Pd[:, :6].contiguous(), sd[:, :6].contiguous(), top3))
    assert _bytes_equal(small[:, first:], Q[:, first:])
    # ... and moves with the sweep, the node, the counter, the seed and the sample
    A_same = Ad.clone()
    A_same[:, 3] = A_same[:, 2]
    for other in (run(sweep=2), run(t=5), run(seed=10), run(inputs=(A_same, Pd, sd, top5), k=3), run(t=4 + (1 << 32))):
        assert not torch.equal(_bits(other[:, first:]), _bits(Q[:, first:]))
    B_same = Ad.clone()
    B_same[1] = B_same[0]
    twin = run(inputs=(B_same, Pd, sd, top5))
    assert not torch.equal(_bits(twin[0, first:]), _bits(twin[1, first:]))
    # no counter is counter 0
    none = ops.pose_graph_propose(Ad, Pd, sd, top5, k, N, 3.0, sweep=1, seed=9)[0]
    assert _bytes_equal(none, run(t=0))


def test_propose_noise_has_the_stated_scale(ahv, ops, dev):
    """4 096 noise slots at sigma = 3 degrees: the squared angle of exp([sigma z]x) is sigma^2 chi^2_3, mean 3 sigma^2 and
    standard deviation sigma^2 sqrt(6 / 4096) of the mean over 4 096 slots = 1.3 % of it: 5 % is a band 3.9 deviations wide."""
    top = ops.PoseGraphTopology(3, None, 0, device=dev)
    P, s = _pairs(ahv, 1, 6, seed=5)
    A = ahv.rotations.haar_rotations_np(3, seed=6).reshape(1, 3, 3, 3)
    D, sigma = top.degree[1], 3.0
    Q = ops.pose_graph_propose(_t(A).to(dev), _t(P).to(dev), _t(s).to(dev), top, 1, 1 + D + 4096, sigma, seed=77)[0]
    ang = tr.geodesic_deg(np.broadcast_to(A[0, 1].astype(np.float64), (4096, 3, 3)), Q[0, 1 + D:].cpu().double().numpy())
    got = float((ang ** 2).mean())
    print("mean squared angle over 4096 slots %.4f deg^2, 3 sigma^2 = %.4f" % (got, 3 * sigma * sigma))
    assert abs(got / (3 * sigma * sigma) - 1.0) <= 0.05
    still = ops.pose_graph_propose(_t(A).to(dev), _t(P).to(dev), _t(s).to(dev), top, 1, 1 + D + 8, 0.0, seed=77)[0]
    assert float(tr.geodesic_deg(np.broadcast_to(A[0, 1].astype(np.float64), (8, 3, 3)), still[0, 1 + D:].cpu().double().numpy()).max()) < 1e-4


# ---- 3. pose_graph_commit ------------------------------------------------------------------------------------------------
def test_commit_is_exact_and_skips_a_sample_without_a_finite_score(ahv, ops, dev):
    B, V, N, k = 5, 4, 37, 2
    A = ahv.rotations.haar_rotations_np(B * V, seed=1).reshape(B, V, 3, 3)
    Q = ahv.rotations.haar_rotations_np(B * N, seed=2).reshape(B, N, 3, 3)
    ns = np.linspace(-1, 1, B * V, dtype=np.float32).reshape(B, V)
    keys = ahv.dist.pack_keys_host(np.array([0.25, np.nan, -0.5, np.inf, -np.inf], np.float32), np.array([36, 3, 0, 5, 7]))
    keys[2] = vr.EMPTY
    wantA, wants = pgr.commit(A, ns, Q, keys, k)
    assert not np.array_equal(wantA[0], A[0]) and np.array_equal(wantA[1:], A[1:])                 # only sample 0 holds a finite score
    Ad, nsd = _t(A).to(dev), _t(ns).to(dev)
    gotA, gots = ops.pose_graph_commit(_t(keys).to(dev), _t(Q).to(dev), Ad, nsd, k)
    assert gotA is Ad and gots is nsd
    assert _bytes_equal(Ad.cpu(), _t(wantA)) and _bytes_equal(nsd.cpu(), _t(wants))


# ---- 4. one node update end to end ------------------------------------------------------------------------------------
def test_one_node_update_against_the_oracle(ahv, ops, oracle, dev, head):
    """The fused row within the project's score bar (1e-4 relative, floor 1e-2) of the oracle's per-edge scores of the SAME
    edge rotations averaged in fp64; the arg-max exact wherever the reference's top two differ by more than that bar."""
    V, N, B, k = 3, 64, 2, 1
    top = ops.PoseGraphTopology(V, None, 0, device=dev)
    D, E = top.degree[k], top.n_edges
    rng = np.random.default_rng(12)
    vs, vt = (rng.standard_normal((B, E) + VOL).astype(np.float32) for _ in range(2))
    P, s = _pairs(ahv, B, E, seed=13)
    A = ahv.rotations.haar_rotations_np(B * V, seed=14).reshape(B, V, 3, 3)
    Ad = _t(A).to(dev)
    Q, Rrel = ops.pose_graph_propose(Ad, _t(P).to(dev), _t(s).to(dev), top, k, N, 4.0, seed=3, n_fresh=8)
    ids = torch.tensor([[e for e, _ in top.incident[k]]] * B, dtype=torch.int32, device=dev)
    src_k, tgt_k = ops.gather_views(_t(vs).to(dev), ids), ops.gather_views(_t(vt).to(dev), ids)
    fused, key = ops.pose_graph_score(src_k, tgt_k, Rrel, *head)
    w = tuple(h.cpu().numpy() for h in head)
    ref = np.zeros((B, D, N))
    Rh = Rrel.cpu().numpy()
    for b in range(B):
        for d, (e, _) in enumerate(top.incident[k]):
            ref[b, d] = oracle.score_hypotheses(vs[b, e][None], vt[b, e][None], Rh[b, d], *w)[0][0]
    want = ref.mean(axis=1)
    got = fused.cpu().double().numpy()
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-2)
    print("one node update: max relative error of the fused row %.3e" % rel.max())
    assert rel.max() < 1e-4
    score, idx = vr.decode(key.cpu().numpy())
    for b in range(B):
        order = np.argsort(-want[b])
        if want[b, order[0]] - want[b, order[1]] > 1e-4 * max(abs(want[b, order[0]]), 1e-2):
            assert idx[b] == order[0]
        assert score[b] == fused[b].max().item()
    # the commit takes that candidate, bit for bit
    ns = torch.zeros((B, V), device=dev)
    before = Ad.clone()
    ops.pose_graph_commit(key, Q, Ad, ns, k)
    for b in range(B):
        assert _bytes_equal(Ad[b, k], Q[b, int(idx[b])]) and ns[b, k].item() == score[b]
    assert _bytes_equal(Ad[:, [0, 2]], before[:, [0, 2]])


# ---- 5. monotonicity ---------------------------------------------------------------------------------------------------
class _Recorder:
    """``ops`` with every commit's slot-0 score and committed score kept on the device."""

    def __init__(self, ops):
        self._ops, self.rows, self.graph = ops, [], None

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def pose_graph_commit(self, key, Q, A, node_score, k):
        out = self._ops.pose_graph_commit(key, Q, A, node_score, k)
        self.rows.append((k, self.graph._fused[:, 0].clone(), node_score[:, k].clone()))
        return out


def _planted(ahv, ops, dev, V, n_bad, seed):
    rot = lambda vol, R: ops.rotate_volume(_t(vol).to(dev), _t(np.asarray(R, np.float32)[None]).to(dev)).cpu().numpy()
    vs, vt, truth, bad = pgr.planted_volumes(rot, ahv.rotations, V, n_bad, seed)
    return _t(vs).to(dev), _t(vt).to(dev), truth, bad


def test_ascent_never_decreases_a_node_score(ahv, ops, dev, head):
    V = 4
    vs, vt, truth, bad = _planted(ahv, ops, dev, V, 2, 5)
    vs, vt = vs.repeat(2, 1, 1, 1, 1, 1), vt.repeat(2, 1, 1, 1, 1, 1)
    rec = _Recorder(ops)
    g = ahv.posegraph.PoseGraph(*head, n_views=V, batch=2, candidates=64, sweeps=2, sigma_deg=(5, 2), seed=2, backend=rec)
    rec.graph = g
    R0 = ops.random_rotations(512, seed=8, device=dev)
    res = g.solve(vs, vt, R0)
    assert len(rec.rows) == 2 * (V - 1)
    for k, slot0, committed in rec.rows:
        assert (committed >= slot0).all(), (k, slot0, committed)      # exactly: slot 0 is the current rotation, bit for bit
    # the mean over ALL edges of the score at the final A against the tree's, one verify_pair launch each
    E = g.E
    mean = lambda A: ops.verify_pair(vs.view((2 * E,) + VOL), vt.view((2 * E,) + VOL), g.relative(A).reshape(2 * E, 1, 3, 3).contiguous(),
                                     *head)[0].view(2, E).double().mean(dim=1)
    final, start = mean(res.A), mean(res.init_A)
    print("mean edge score: tree %s -> joint %s" % (start.tolist(), final.tolist()))
    assert (final >= start).all()


# ---- 6. the planted graph on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_graph_on_the_device(ahv, ops, dev, head, seed):
    """V = 5, 3 bad edges, 4 096 shared Haar hypotheses for the pairwise stage, 256 candidates per node update, 8 sweeps.
    Bar 1: the joint solution's LARGEST relative-rotation error over all ordered pairs, bad edges included, is below the MEDIAN
    pairwise arg-max error over the clean edges.  Bar 2: no bad edge is a tree edge.  And the captured solve gives the eager
    solve's bytes for the same counter."""
    V, n_bad = 5, 3
    vs, vt, truth, bad = _planted(ahv, ops, dev, V, n_bad, seed)
    R0 = ops.random_rotations(4096, seed=100 + seed, device=dev)
    make = lambda graph: ahv.posegraph.PoseGraph(*head, n_views=V, candidates=256, sweeps=8, sigma_deg=pgr.SIGMA_DEG, seed=seed,
                                                 use_graph=graph)
    eager = make(False)
    res = eager.solve(vs, vt, R0)
    fig = pgr.planted_figures(res.A[0].cpu().numpy(), res.pair_R[0].cpu().numpy(), res.parent_edge[0].cpu().numpy(), truth, bad, V)
    tree = pgr.planted_figures(res.init_A[0].cpu().numpy(), res.pair_R[0].cpu().numpy(), res.parent_edge[0].cpu().numpy(), truth, bad, V)
    clean = [e for e in range(V * (V - 1)) if e not in bad]
    print("planted V=%d bad=%s seed=%d: joint max %.3f median %.3f | tree max %.3f | pairwise clean median %.3f max %.3f | bad %s | "
          "scores clean min %.3f bad max %.3f" % (V, bad, seed, fig["joint_max"], fig["joint_median"], tree["joint_max"],
                                                  fig["pair_clean_median"], fig["pair_clean_max"],
                                                  ["%.1f" % x for x in fig["pair_bad"]], float(res.pair_score[0, clean].min()),
                                                  float(res.pair_score[0, bad].max())))
    assert fig["joint_max"] < fig["pair_clean_median"], fig
    assert fig["bad_in_tree"] == [], fig
    first = res.A.clone()
    captured = make(True)
    got = captured.solve(vs, vt, R0)
    assert int(captured.counter[0]) == int(eager.counter[0]) == 1
    assert _bytes_equal(got.A, first) and _bytes_equal(got.init_A, res.init_A) and _bytes_equal(got.node_score, res.node_score)
    # a replay moves the counter on the device and draws new noise; the eager object's second solve draws the same
    again, second = captured.solve(vs, vt, R0).A.clone(), eager.solve(vs, vt, R0).A
    assert int(captured.counter[0]) == 2 and _bytes_equal(again, second) and not _bytes_equal(again, first)
