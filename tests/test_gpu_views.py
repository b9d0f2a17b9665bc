"""Multi-view verification on the GPU: ``ahv_view_rotations_f32`` / ``ahv_fuse_view_scores_f32`` through ``ops.view_rotations``,
``ops.fuse_view_scores`` and ``ops.verify_views`` against the numpy fp64 reference (tests/views_reference.py) and the fixture
the reference's own code produced (G13 ``multiview``).

Tolerance of a finite fused score: ``4 (V + 2) 2^-24 * sum_v g w |s| / sum_v g w`` -- the rounding of V products, V adds and one
division (each at most 2^-24 relative to a partial sum that never exceeds sum g w |s|; the denominator's V adds likewise), with
a factor 4 of slack.  The participation decision t >= tau is NOT compared at the threshold: hypotheses whose fp64 t comes within
2e-4 of tau for any view are replaced (from a second Haar stream) when the inputs are made, and every comparison first asserts
that the reference's smallest |t - tau| is at least 1e-4 -- fp32 rounding moves t by ~1e-6."""
import numpy as np
import pytest
import torch

from . import modes_reference as mr
from . import posterior_reference as pr
from . import views_reference as vr
from .conftest import load_golden

pytestmark = pytest.mark.gpu

SCORE_RTOL, SCORE_FLOOR = 1e-4, 1e-2   # the project's score bar (tests/test_gpu_parity.py)
THETA, MARGIN = 60.0, 1e-4
NS, VS, BS = (1, 3, 4, 5, 1021, 1024, 1025, 2049, 4100), (1, 2, 3, 16), (1, 3)


@pytest.fixture(scope="module")
def dev(ahv):
    ahv._lib.load()  # raises if libahv_hip.so is missing: no fallback
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def relerr(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), SCORE_FLOOR)))


def clear_of_threshold(Q, A, spare, theta=THETA, guard=2 * MARGIN):
    """Q (B,N,3,3) with every hypothesis whose t to some view of its sample lies within ``guard`` of tau replaced, in order,
    by the next rotation of ``spare`` that is clear of tau for all of that sample's views."""
    tau = float(vr.tau_of(theta))
    Q = Q.copy()
    nxt = 0
    for b in range(Q.shape[0]):
        t = np.einsum("nij,vij->vn", Q[b].astype(np.float64), A[b].astype(np.float64))
        for n in np.flatnonzero((np.abs(t - tau) < guard).any(axis=0)):
            while True:
                c = spare[nxt]
                nxt += 1
                if (np.abs(np.einsum("ij,vij->v", c.astype(np.float64), A[b].astype(np.float64)) - tau) >= guard).all():
                    Q[b, n] = c
                    break
    return Q


_cases = {}


def case(ahv, dev, B, V, N):
    """(scores (B,V,N), Q (B,N,3,3), A (B,V,3,3), Q_shared (N,3,3)) of a shape, made once and never modified: N(0,1) scores with
    a few +-inf and NaN entries, Haar hypotheses from ``ops.random_rotations`` (kept clear of the 60-degree threshold; the
    shared set: sample 0's, kept clear for the views of every sample), Haar view poses."""
    key = (B, V, N)
    if key not in _cases:
        seed = 1000 * B + 10 * V + N
        rng = np.random.default_rng(seed)
        s = rng.standard_normal((B, V, N)).astype(np.float32)
        k = min(4, (B * V * N) // 2)
        flat = rng.choice(B * V * N, size=k, replace=False)
        s.reshape(-1)[flat] = np.array([np.inf, -np.inf, np.nan, np.inf], np.float32)[:k]
        A = ahv.rotations.haar_rotations_np(B * V, seed=seed + 1).reshape(B, V, 3, 3)
        pool = ahv.ops.random_rotations(B * N + 1024, seed=seed, device=dev).cpu().numpy()
        raw, spare = pool[:B * N].reshape(B, N, 3, 3), pool[B * N:]
        Q = clear_of_threshold(raw, A, spare[:512])
        Q_shared = clear_of_threshold(raw[:1], A.reshape(1, B * V, 3, 3), spare[512:])[0]
        _cases[key] = (s, Q, A, Q_shared)
    return _cases[key]


def weights_for(V):
    """Unequal weights with an absent view wherever there is more than one."""
    w = [0.5 + 0.25 * v for v in range(V)]
    if V > 1:
        w[V // 2] = 0.0
    return w


def check_fused(got, want, scale, V, label):
    """NaN / +inf / -inf masks equal; finite values within the bound.  Prints the figures before it asserts."""
    got = np.asarray(got, np.float64)
    for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got), f(want)), (label, name)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    bound = 4.0 * (V + 2) * 2.0 ** -24 * scale[fin]
    err = np.abs(got[fin] - want[fin])
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: max |err| %.3e, worst err / bound %.3f" % (label, float(err.max()), worst))
    assert np.all(err <= bound), (label, worst)
    return worst


# ---- fuse_view_scores on given score arrays -------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("N", NS)
def test_fuse_against_the_reference(ahv, dev, N, V):
    ops = ahv.ops
    for B in BS:
        s, Q, A, Q_shared = case(ahv, dev, B, V, N)
        sg, Ag = T(s, dev), T(A, dev)
        for per in ((False,) if B == 1 else (True, False)):       # per-sample Q (B,N,3,3), or one set (N,3,3) shared by the batch
            Qn = Q if per else Q_shared
            Qg = T(Qn, dev)
            for w in (None, weights_for(V)):
                for theta in (None, THETA):
                    sw = s
                    if w is not None and V > 1:                   # the absent view's scores are never read: poison them
                        sw = s.copy()
                        sw[:, V // 2] = np.nan
                    want, scale, g, margin = vr.fuse(sw, Qn, A, w, theta)
                    assert margin >= MARGIN
                    fused, key = ops.fuse_view_scores(T(sw, dev) if sw is not s else sg, Qg, Ag, w, theta, n_offset=3)
                    label = "N=%d V=%d B=%d per=%s w=%s theta=%s" % (N, V, B, per, w is not None, theta)
                    check_fused(fused.cpu().numpy(), want, scale, V, label)
                    assert torch.equal(key, ops.argmax(fused, 3, return_key=True)), label
                    if theta is not None and N >= 1021:
                        assert 0 < g.sum() < g.size                # the limit decides something on these inputs
                    _, key_only = ops.fuse_view_scores(T(sw, dev) if sw is not s else sg, Qg, Ag, w, theta, n_offset=3,
                                                       want_scores=False)
                    assert torch.equal(key_only, key), label


def test_key_tie_offset_and_merge(ahv, dev):
    """Two equal rows of Q with equal scores: the lowest index wins; the key is ``ops.argmax`` of the fused row bit for bit,
    with ``n_offset``; merging into a key that already holds something larger leaves it."""
    ops = ahv.ops
    B, V, N = 3, 3, 4100
    s, Q, A, _ = case(ahv, dev, B, V, N)
    s, Q = np.nan_to_num(s, nan=0.0, posinf=1.0, neginf=-1.0), Q.copy()
    s[:, :, 3000] = s[:, :, 1500] = 7.0
    Q[:, 3000] = Q[:, 1500]
    for theta in (None, THETA):
        want, scale, g, margin = vr.fuse(s, Q, A, None, theta)
        assert margin >= MARGIN
        fused, key = ops.fuse_view_scores(T(s, dev), T(Q, dev), T(A, dev), None, theta, n_offset=1000)
        assert torch.equal(key, ops.argmax(fused, 1000, return_key=True))
        sc, idx = ops.unpack_best(key)
        assert torch.equal(fused[:, 1500], fused[:, 3000])
        ref_idx = vr.decode(vr.best_keys(fused.cpu().numpy(), 1000))[1]
        assert idx.cpu().tolist() == ref_idx.tolist()
        if theta is None:
            assert idx.cpu().tolist() == [2500] * B and sc.cpu().tolist() == [7.0] * B
        # merge: a key that already holds a larger score stays; an EMPTY one takes this call's
        big = ops.argmax(torch.full((B, 1), 9.0, device=dev), 77, return_key=True)
        _, merged = ops.fuse_view_scores(T(s, dev), T(Q, dev), T(A, dev), None, theta, n_offset=1000, want_scores=False,
                                         best_key=big.clone())
        assert torch.equal(merged, big)
        _, reset = ops.fuse_view_scores(T(s, dev), T(Q, dev), T(A, dev), None, theta, n_offset=1000, want_scores=False,
                                        best_key=big.clone(), reset_best=True)
        assert torch.equal(reset, key)


def test_chunks_compose_and_runs_repeat(ahv, dev):
    ops = ahv.ops
    B, V, N, CUT, OFF = 3, 3, 4100, 1500, 40
    s, Q, A, _ = case(ahv, dev, B, V, N)
    sg, Qg, Ag = T(s, dev), T(Q, dev), T(A, dev)
    for w, theta in ((None, None), (weights_for(V), THETA)):
        fused, key = ops.fuse_view_scores(sg, Qg, Ag, w, theta, n_offset=OFF)
        f1, k = ops.fuse_view_scores(sg[:, :, :CUT], Qg[:, :CUT], Ag, w, theta, n_offset=OFF)
        f2, k2 = ops.fuse_view_scores(sg[:, :, CUT:], Qg[:, CUT:], Ag, w, theta, n_offset=OFF + CUT, best_key=k)
        assert k2 is k and torch.equal(k, key)
        assert torch.equal(torch.cat([f1, f2], dim=1).view(torch.int32), fused.view(torch.int32))
        again, key_again = ops.fuse_view_scores(sg, Qg, Ag, w, theta, n_offset=OFF)
        assert torch.equal(again.view(torch.int32), fused.view(torch.int32)) and torch.equal(key_again, key)


def test_fuse_in_a_captured_graph(ahv, dev):
    """The weights travel in the kernel's arguments: a captured call replays with them and reads no host memory."""
    ops = ahv.ops
    s, Q, A, _ = case(ahv, dev, 3, 3, 1025)
    sg, Qg, Ag = T(s, dev), T(Q, dev), T(A, dev)
    w = weights_for(3)
    ref, ref_key = ops.fuse_view_scores(sg, Qg, Ag, w, THETA)
    key = torch.empty(3, dtype=torch.int64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused, _ = ops.fuse_view_scores(sg, Qg, Ag, w, THETA, best_key=key, reset_best=True)
    del w
    for _ in range(2):
        fused.zero_()
        key.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(fused.view(torch.int32), ref.view(torch.int32)) and torch.equal(key, ref_key)


# ---- view_rotations ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 5, 1025])
def test_view_rotations_both_layouts(ahv, dev, N):
    B, V = 3, 3
    _, Q, A, _ = case(ahv, dev, B, V, 1025)
    Q = Q[:, :N]
    for Qn in (Q, Q[1]):
        got = ahv.ops.view_rotations(T(Qn, dev), T(A, dev))
        want = vr.view_rotations(Qn, A)
        assert got.shape == (B, V, N, 3, 3)
        err = float(np.max(np.abs(got.cpu().numpy() - want)))
        print("view_rotations N=%d %s: max |err| %.2e" % (N, "per-sample" if Qn.ndim == 4 else "shared", err))
        assert err <= 1e-6
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 1, 3, 3))
    assert torch.equal(ahv.ops.view_rotations(T(Q, dev), T(eye, dev))[:, 0], T(Q, dev))     # A = I: Q itself, bit for bit


# ---- verify_views end to end ------------------------------------------------------------------------------------------------

def test_verify_views_against_the_multiview_fixture(ahv, dev):
    ops = ahv.ops
    g = load_golden("multiview")
    refs, query, Q, A, W1, W2, b2 = (T(g[k], dev) for k in ("vol_refs", "vol_query", "Q", "A", "W1", "W2", "b2"))
    fused, key, per_view = ops.verify_views(refs, query, Q, A, W1, W2, b2, want_view_scores=True)
    print("G13: per-view rel err %.2e, fused rel err %.2e" % (relerr(per_view.cpu().numpy(), g["scores"]),
                                                              relerr(fused.cpu().numpy(), g["fused"])))
    assert relerr(per_view.cpu().numpy(), g["scores"]) <= SCORE_RTOL
    assert relerr(fused.cpu().numpy(), g["fused"]) <= SCORE_RTOL
    score, idx, R_pred = ops.select_rotation(key, Q)
    assert idx.cpu().tolist() == g["best_idx"].tolist()
    assert torch.equal(R_pred, Q[idx]) and torch.equal(score, fused[torch.arange(2, device=dev), idx])
    assert relerr(score.cpu().numpy(), g["best"]) <= SCORE_RTOL
    _, key_only = ops.verify_views(refs, query, Q, A, W1, W2, b2, want_scores=False)
    assert torch.equal(key_only, key)
    # the split-f16 scorer through the same path
    f16, k16 = ops.verify_views(refs, query, Q, A, W1, W2, b2, split_f16=True)
    assert relerr(f16.cpu().numpy(), g["fused"]) <= SCORE_RTOL and ops.unpack_best(k16)[1].cpu().tolist() == g["best_idx"].tolist()
    # one view: the fused row is verify_pair's score row for that pair, bit for bit
    for v in range(3):
        f1, k1 = ops.verify_views(refs[:, v:v + 1], query, Q, A[:, v:v + 1], W1, W2, b2)
        R1 = ops.view_rotations(Q, A[:, v:v + 1])[:, 0]
        s1, kp = ops.verify_pair(refs[:, v].contiguous(), query, R1, W1, W2, b2)
        assert torch.equal(f1, s1) and torch.equal(k1, kp), v
    # the module's method: this head's weights, the inference rule of verify_hypotheses
    fa = ahv.aligner.Feature_Aligner(in_channel=64, mid_channel=32, out_channel=32, n_heads=4, depth=1).to(dev).eval()
    with torch.no_grad():
        c1, c2 = fa.feature_embedding_2d[0], fa.feature_embedding_2d[2]
        c1.weight.copy_(W1.reshape(c1.weight.shape))
        c2.weight.copy_(W2.reshape(c2.weight.shape))
        c2.bias.copy_(b2)
    fm, km = fa.verify_views(refs, query, Q, A)
    assert torch.equal(fm, fused) and torch.equal(km, key) and not fm.requires_grad


def test_planted_pose_is_found(ahv, dev):
    """B = 1, V = 4, N = 4 100: every reference volume is ``ops.rotate_volume`` of one random volume by its A_v, the query the
    same volume rotated by a pose that Q contains once: the fused arg-max is that hypothesis."""
    ops = ahv.ops
    g = load_golden("score_n128")
    W1, W2, b2 = (T(g[k], dev) for k in ("W1", "W2", "b2"))
    V, N, PLANT = 4, 4100, 2345
    X = torch.from_numpy(np.random.default_rng(17).standard_normal((1, 16, 8, 8, 8)).astype(np.float32)).to(dev)
    ax = lambda axis, deg: torch.from_numpy(pr_axis(axis, deg)).to(dev)
    A = torch.stack([ax("z", 25.0), ax("x", -30.0) @ ax("y", 20.0), ax("y", 35.0) @ ax("z", -15.0), ax("x", 30.0)])[None]
    Q_true = (ax("y", 15.0) @ ax("x", 10.0))[None]
    Q = T(ahv.rotations.haar_rotations_np(N, seed=23), dev)
    Q[PLANT] = Q_true[0]
    refs = ops.rotate_volume(X.expand(V, -1, -1, -1, -1), A[0])[None]
    query = ops.rotate_volume(X, Q_true)
    fused, key, per_view = ops.verify_views(refs, query, Q, A, W1, W2, b2, want_view_scores=True)
    score, idx, R_pred = ops.select_rotation(key, Q)
    top2 = torch.topk(fused[0], 2).values
    print("planted pose: idx %d score %.4f lead %.4f per-view arg-max %s" % (idx.item(), score.item(), (top2[0] - top2[1]).item(),
                                                                            per_view[0].argmax(dim=1).tolist()))
    assert idx.item() == PLANT and torch.equal(R_pred, Q_true)


def pr_axis(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m, dtype=np.float32)


# ---- the fused row downstream ----------------------------------------------------------------------------------------------

def test_downstream_ops_take_the_fused_row(ahv, dev):
    """``topk``, ``topk_modes`` and ``pose_posterior`` on a fused row with Q as its matrices, against their own references at
    N = 1025, K = 4 (planted-peak scores, each view's copy perturbed; anchors = the modes at 30 degrees)."""
    from .test_gpu_posterior import as_np, check
    ops = ahv.ops
    N, B, V, K, ANGLE = 1025, 3, 3, 4, 30.0
    s, R, _ = pr.make_inputs(N, B, False, 0, K=K, angle_deg=ANGLE)
    rng = np.random.default_rng(31)
    views = (s[:, None] + 0.01 * rng.standard_normal((B, V, N))).astype(np.float32)
    A = ahv.rotations.haar_rotations_np(B * V, seed=32).reshape(B, V, 3, 3)
    fused, key = ops.fuse_view_scores(T(views, dev), T(R, dev), T(A, dev), [1.0, 2.0, 1.0])
    f = fused.cpu().numpy()
    want, scale, _, _ = vr.fuse(views, R, A, [1.0, 2.0, 1.0])
    check_fused(f, want, scale, V, "downstream input")
    Rg = T(R, dev)
    # K best: the stable descending sort
    keys = ops.topk(fused, K)
    order = torch.sort(torch.from_numpy(f), dim=1, descending=True, stable=True).indices.numpy()[:, :K]
    assert np.array_equal(mr.indices(keys.cpu().numpy()), order) and torch.equal(keys[:, 0], key)
    # distinct modes
    want_modes, margin = mr.select_modes(f, R, K, ANGLE)
    assert margin >= MARGIN
    modes = ops.topk_modes(fused, Rg, K, ANGLE)
    assert np.array_equal(modes.cpu().numpy(), want_modes)
    # posterior with the modes as anchors
    m_s, m_i, m_R = ops.select_topk(modes, Rg)
    for temp in (0.1, 0.02):
        want_post, margin = pr.posterior(f, R, m_R.cpu().numpy(), ANGLE, temp)
        post = ops.pose_posterior(fused, Rg, temp, anchors=m_R, min_angle_deg=ANGLE)
        check(as_np(post), want_post, margin, "fused row T=%g:" % temp)
