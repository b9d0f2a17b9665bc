"""Angle-limited multi-view verification, compact, on the GPU: ``ahv_view_rotations_compact_f32`` /
``ahv_fuse_view_scores_compact_f32`` through ``ops.view_rotations_compact``, ``ops.fuse_view_scores_compact`` and
``ops.verify_views(compact=True)``.

Two yardsticks.  Against the numpy reference (tests/views_compact_reference.py, tests/views_reference.py) the inputs are those of
tests/test_gpu_views.py -- theta = 60 degrees, hypotheses kept clear of the threshold -- and every comparison first asserts that
the reference's smallest |t - tau| is at least MARGIN = 1e-4 (fp32 rounding moves t by ~1e-6); fused scores are held to
``check_fused``'s bound.  Against the DENSE GPU path no margin is needed and none is used: both sides evaluate the same fp32 t
with the same fma chain, and a score is a function of (volumes, head weights, R_n) alone, so the compact path has to reproduce
the dense fused row and key bit for bit.  That equality is part of what is under test."""
import numpy as np
import pytest
import torch

from . import views_compact_reference as vcr
from . import views_reference as vr
from .conftest import load_golden
from .test_gpu_views import BS, MARGIN, NS, THETA, VS, T, case, check_fused, pr_axis, weights_for

pytestmark = pytest.mark.gpu

E2E_SHAPES = ((1, 1, 5), (3, 3, 1025), (1, 16, 1025), (3, 3, 4100))


@pytest.fixture(scope="module")
def dev(ahv):
    ahv._lib.load()  # raises if libahv_hip.so is missing: no fallback
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def head(dev):
    g = load_golden("score_n128")
    return tuple(T(g[k], dev) for k in ("W1", "W2", "b2"))


def bits(t):
    """The bit pattern of a float32 tensor / array: NaN equals NaN, -0 differs from +0."""
    return t.view(torch.int32) if isinstance(t, torch.Tensor) else np.ascontiguousarray(t, np.float32).view(np.int32)


_volumes = {}


def volumes(dev, B, V):
    """Random reference and query volumes of a shape, made once."""
    if (B, V) not in _volumes:
        rng = np.random.default_rng(100 * B + V)
        _volumes[(B, V)] = (T(rng.standard_normal((B, V, 16, 8, 8, 8)).astype(np.float32), dev),
                            T(rng.standard_normal((B, 16, 8, 8, 8)).astype(np.float32), dev))
    return _volumes[(B, V)]


def same_as_dense(ops, refs, query, Q, A, hd, label, **kw):
    """``verify_views`` dense and compact with the same keywords: fused row, key and expanded per-view scores bit for bit."""
    fd, kd, sd = ops.verify_views(refs, query, Q, A, *hd, want_view_scores=True, **kw)
    fc, kc, sc, counts = ops.verify_views(refs, query, Q, A, *hd, want_view_scores=True, compact=True, want_counts=True, **kw)
    assert torch.equal(bits(fc), bits(fd)), label
    assert torch.equal(kc, kd), label
    assert sc.shape == sd.shape
    took = ~torch.isnan(sc)
    assert torch.equal(bits(sc)[took], bits(sd)[took]), label
    assert torch.equal(took.sum(dim=2), counts), label              # NaN exactly where the pair was not scored (scores are finite)
    _, k_only = ops.verify_views(refs, query, Q, A, *hd, want_scores=False, compact=True, **kw)
    assert torch.equal(k_only, kd), label
    return fd, kd, sd, counts


# ---- 1. the compaction against the reference -------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("N", NS)
def test_compaction_against_the_reference(ahv, dev, N, V):
    ops = ahv.ops
    for B in BS:
        _, Q, A, Q_shared = case(ahv, dev, B, V, N)
        Ag = T(A, dev)
        for per in ((False,) if B == 1 else (True, False)):       # per-sample Q (B,N,3,3), or one set (N,3,3) shared by the batch
            Qn = Q if per else Q_shared
            Qg = T(Qn, dev)
            dense = ops.view_rotations(Qg, Ag).cpu().numpy()
            for w in (None, weights_for(V)):
                label = "N=%d V=%d B=%d per=%s w=%s" % (N, V, B, per, w is not None)
                slot, counts, g, margin = vcr.compact(Qn, A, THETA, w)
                assert margin >= MARGIN
                R, slot_g, counts_g = ops.view_rotations_compact(Qg, Ag, THETA, w)
                M = max(1, int(counts.max()))
                assert R.shape == (B, V, M, 3, 3) and slot_g.dtype == torch.int32 and counts_g.dtype == torch.int64
                assert np.array_equal(counts_g.cpu().numpy(), counts), label
                assert np.array_equal(slot_g.cpu().numpy(), slot), label
                # R[b,v,m] = the dense matrix of the n with slot m, bit for bit; the identity in every slot past the count
                assert np.array_equal(bits(R.cpu().numpy()), bits(vcr.gather(dense, slot, M))), label
                if w is not None and V > 1:
                    assert not counts[:, V // 2].any()             # the absent view
                if N >= 1021:
                    assert 0 < counts.sum() < B * V * N            # the limit decides something on these inputs
                # a caller's capacity above every count: the same lists, more padding, no host read
                cap = min(N, M + 5)
                R2, slot2, counts2 = ops.view_rotations_compact(Qg, Ag, THETA, w, capacity=cap)
                assert torch.equal(slot2, slot_g) and torch.equal(counts2, counts_g), label
                assert np.array_equal(bits(R2.cpu().numpy()), bits(vcr.gather(dense, slot, cap))), label


# ---- 2. the compact fuse on given scores -----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("N", NS)
def test_compact_fuse_against_the_dense_fuse_and_the_reference(ahv, dev, N, V):
    ops = ahv.ops
    for B in BS:
        _, Q, A, Q_shared = case(ahv, dev, B, V, N)
        Ag = T(A, dev)
        for per in ((False,) if B == 1 else (True, False)):
            Qn = Q if per else Q_shared
            Qg = T(Qn, dev)
            for w in (None, weights_for(V)):
                label = "N=%d V=%d B=%d per=%s w=%s" % (N, V, B, per, w is not None)
                _, slot_g, counts_g = ops.view_rotations_compact(Qg, Ag, THETA, w)
                slot, counts = slot_g.cpu().numpy(), counts_g.cpu().numpy()
                M = max(1, int(counts.max()))
                rng = np.random.default_rng(7 * N + V + B)
                cs = rng.standard_normal((B, V, M)).astype(np.float32)
                live = np.flatnonzero((np.arange(M)[None, None] < counts[:, :, None]).reshape(-1))
                if live.size:
                    k = min(4, live.size)
                    cs.reshape(-1)[rng.choice(live, size=k, replace=False)] = np.array([np.inf, -np.inf, np.nan, np.inf], np.float32)[:k]
                cs[np.arange(M)[None, None] >= counts[:, :, None]] = np.nan     # past a list's end: never read
                sd = vcr.scatter(cs, slot, np.nan)                               # dense layout, every other pair poisoned
                fd, kd = ops.fuse_view_scores(T(sd, dev), Qg, Ag, w, THETA, n_offset=3)
                fc, kc = ops.fuse_view_scores_compact(T(cs, dev), slot_g, w, n_offset=3)
                assert torch.equal(bits(fc), bits(fd)) and torch.equal(kc, kd), label
                want, scale, g, margin = vr.fuse(sd, Qn, A, w, THETA)
                assert margin >= MARGIN
                assert np.array_equal(g, slot >= 0), label
                check_fused(fc.cpu().numpy(), want, scale, V, label)
                assert torch.equal(kc, ops.argmax(fc, 3, return_key=True)), label
                none, k_only = ops.fuse_view_scores_compact(T(cs, dev), slot_g, w, n_offset=3, want_scores=False)
                assert none is None and torch.equal(k_only, kc), label


# ---- 3. end to end, bit for bit --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,V,N", E2E_SHAPES)
def test_verify_views_compact_equals_dense_bit_for_bit(ahv, dev, head, B, V, N):
    ops = ahv.ops
    _, Q, A, Q_shared = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Ag = T(A, dev)
    for Qn in (Q, Q_shared):
        Qg = T(Qn, dev)
        for kw in ({"max_view_angle_deg": 60.0}, {"max_view_angle_deg": 60.0, "weights": weights_for(V), "n_offset": 11},
                   {"max_view_angle_deg": 60.0, "split_f16": True}, {"max_view_angle_deg": 90.0},
                   {"max_view_angle_deg": 90.0, "split_f16": True}):
            fd, kd, sd, counts = same_as_dense(ops, refs, query, Qg, Ag, head, "B=%d V=%d N=%d %s %s" % (B, V, N, Qn.ndim, kw), **kw)
            if N >= 1025:
                assert 0 < int(counts.sum()) < B * V * N
    # the module's method: this head's weights, the keywords forwarded
    W1, W2, b2 = head
    fa = ahv.aligner.Feature_Aligner(in_channel=64, mid_channel=32, out_channel=32, n_heads=4, depth=1).to(dev).eval()
    with torch.no_grad():
        c1, c2 = fa.feature_embedding_2d[0], fa.feature_embedding_2d[2]
        c1.weight.copy_(W1.reshape(c1.weight.shape))
        c2.weight.copy_(W2.reshape(c2.weight.shape))
        c2.bias.copy_(b2)
    Qg = T(Q, dev)
    fd, kd = ops.verify_views(refs, query, Qg, Ag, W1, W2, b2, max_view_angle_deg=60.0)
    fm, km, cm = fa.verify_views(refs, query, Qg, Ag, max_view_angle_deg=60.0, compact=True, want_counts=True)
    assert torch.equal(bits(fm), bits(fd)) and torch.equal(km, kd) and not fm.requires_grad and cm.shape == (B, V)


# ---- 4. overflow is visible and deterministic ------------------------------------------------------------------------------

def test_overflow_is_visible_and_deterministic(ahv, dev, head):
    ops = ahv.ops
    B, V, N = 3, 3, 4100
    _, Q, A, _ = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Qg, Ag = T(Q, dev), T(A, dev)
    fd, kd, sd = ops.verify_views(refs, query, Qg, Ag, *head, max_view_angle_deg=THETA, want_view_scores=True)
    _, _, counts_full = ops.view_rotations_compact(Qg, Ag, THETA)
    cap = int(counts_full.max()) - 3
    want_slot, want_counts, g, margin = vcr.compact(Q, A, THETA, capacity=cap)
    assert margin >= MARGIN and cap >= 1 and (want_counts > cap).any()
    for _ in range(2):
        fc, kc, sc, counts = ops.verify_views(refs, query, Qg, Ag, *head, max_view_angle_deg=THETA, want_view_scores=True,
                                              compact=True, capacity=cap, want_counts=True)
        assert torch.equal(counts, counts_full) and np.array_equal(counts.cpu().numpy(), want_counts)   # never clipped
        R, slot, _ = ops.view_rotations_compact(Qg, Ag, THETA, capacity=cap)
        slot = slot.cpu().numpy()
        assert R.shape[2] == cap and np.array_equal(slot, want_slot)
        over = slot == vcr.OVERFLOW
        for b in range(B):
            for v in range(V):              # exactly the last participating n of each overflowing (b, v)
                n_in = np.flatnonzero(g[b, v])
                assert np.array_equal(np.flatnonzero(over[b, v]), n_in[cap:])
        assert over.sum() == np.maximum(want_counts - cap, 0).sum() > 0
        # the dense fuse with those pairs' views masked out: per pattern of masked views one dense call with their weights zero
        pattern = (over << np.arange(V)[None, :, None]).sum(axis=1)                  # (B,N)
        want = torch.empty_like(fd)
        for p in np.unique(pattern):
            w = [0.0 if (p >> v) & 1 else 1.0 for v in range(V)]
            row = ops.fuse_view_scores(sd, Qg, Ag, w, THETA)[0] if any(w) else torch.full_like(fd, -np.inf)
            at = T(pattern == p, dev)
            want[at] = row[at]
        assert not torch.equal(bits(want), bits(fd))                                 # the overflow changed something
        assert torch.equal(bits(fc), bits(want)) and torch.equal(kc, ops.argmax(want, 0, return_key=True))
        scored = T(slot >= 0, dev)
        assert torch.equal(bits(sc)[scored], bits(sd)[scored]) and torch.isnan(sc[~scored]).all()


# ---- 5. edge sets ----------------------------------------------------------------------------------------------------------

def test_a_limit_that_excludes_every_pair(ahv, dev, head):
    ops = ahv.ops
    Q = ahv.rotations.haar_rotations_np(64, seed=7)
    A = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), (1, 2, 3, 3)))
    ang = np.degrees(np.arccos(np.clip((np.trace(Q.astype(np.float64), axis1=1, axis2=2) - 1) / 2, -1, 1)))
    theta = float(ang.min()) * 0.5
    refs, query = volumes(dev, 1, 2)
    Qg, Ag = T(Q, dev), T(A, dev)
    R, slot, counts = ops.view_rotations_compact(Qg, Ag, theta)
    assert R.shape == (1, 2, 1, 3, 3) and torch.equal(R[0, :, 0], torch.eye(3, device=dev).expand(2, 3, 3))    # M = 1: identities
    assert counts.tolist() == [[0, 0]] and bool((slot == vcr.EXCLUDED).all())
    fd, kd, _, _ = same_as_dense(ops, refs, query, Qg, Ag, head, "all excluded", max_view_angle_deg=theta)
    fc, kc = ops.verify_views(refs, query, Qg, Ag, *head, max_view_angle_deg=theta, compact=True)
    assert bool((fc == -np.inf).all()) and ops.unpack_best(kc)[1].tolist() == [0] and ops.unpack_best(kc)[0].tolist() == [-np.inf]


def dense_participation(ops, Qg, Ag, theta, dev):
    """g (B,V,N) as the DENSE fuse kernel decides it: view by view, ones for scores, -inf where the view does not take part."""
    B, V = Ag.shape[:2]
    N = Qg.shape[-3]
    ones = torch.ones((B, 1, N), device=dev)
    return torch.stack([ops.fuse_view_scores(ones, Qg, Ag[:, v:v + 1].contiguous(), None, theta)[0] == 1.0 for v in range(V)], dim=1)


def test_nearly_everything_in_and_thresholds_without_a_margin(ahv, dev, head):
    """theta = 179 degrees: nearly every pair takes part (Haar share 0.989), M reaches N or nearly.  Then raw Haar sets, NOT
    kept clear of any threshold, at 60 / 90 / 150 degrees: the slot map is the dense kernel's own decision, pair for pair."""
    ops = ahv.ops
    B, V, N = 3, 3, 1025
    _, Q, A, _ = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Qg, Ag = T(Q, dev), T(A, dev)
    _, slot, counts = ops.view_rotations_compact(Qg, Ag, 179.0)
    print("theta 179: counts", counts.cpu().tolist())
    assert bool((counts >= 0.95 * N).all()) and bool((counts <= N).all())
    assert torch.equal(slot >= 0, dense_participation(ops, Qg, Ag, 179.0, dev))
    same_as_dense(ops, refs, query, Qg, Ag, head, "theta 179", max_view_angle_deg=179.0)
    all_in = ops.view_rotations_compact(Qg[:, :1].expand(B, N, 3, 3).contiguous(), Qg[:, :1].expand(B, V, 3, 3).contiguous(), 60.0)
    assert bool((all_in[2] == N).all()) and torch.equal(all_in[1], torch.arange(N, dtype=torch.int32, device=dev).expand(B, V, N))
    raw = ops.random_rotations(B * 4100, seed=99, device=dev).reshape(B, 4100, 3, 3)
    for theta in (60.0, 90.0, 150.0):
        _, slot, counts = ops.view_rotations_compact(raw, Ag, theta)
        g = dense_participation(ops, raw, Ag, theta, dev)
        assert torch.equal(slot >= 0, g) and torch.equal(counts, g.sum(dim=2))
        share, p = float(g.float().mean()), ops.haar_view_fraction(theta)
        print("theta %g: share %.4f, Haar %.4f" % (theta, share, p))
        assert abs(share - p) <= 6.0 * np.sqrt(p * (1 - p) / g.numel())


def test_a_nan_entry_in_a_hypothesis(ahv, dev, head):
    ops = ahv.ops
    B, V, N = 3, 3, 1025
    _, Q, A, _ = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Ag = T(A, dev)
    _, slot0, counts0 = ops.view_rotations_compact(T(Q, dev), Ag, 90.0)
    n_in = int(torch.nonzero(slot0[1, 0] >= 0)[0])  # a hypothesis of sample 1 that takes part for view 0
    Qn = Q.copy()
    Qn[1, n_in, 1, 2] = np.nan                      # ... now out for every view of its sample
    Qg = T(Qn, dev)
    R, slot, counts = ops.view_rotations_compact(Qg, Ag, 90.0)
    assert bool((slot[1, :, n_in] == vcr.EXCLUDED).all()) and not bool(torch.isnan(R).any())
    assert counts[1, 0].item() == counts0[1, 0].item() - 1 and torch.equal(counts[0], counts0[0])
    assert torch.equal(slot[1, 0, n_in + 1:][slot[1, 0, n_in + 1:] >= 0], slot0[1, 0, n_in + 1:][slot0[1, 0, n_in + 1:] >= 0] - 1)
    fd, kd, _, _ = same_as_dense(ops, refs, query, Qg, Ag, head, "NaN in Q", max_view_angle_deg=90.0)
    assert fd[1, n_in].item() == -np.inf


def test_key_tie_offset_and_merge(ahv, dev):
    """Two equal rows of Q with equal scores: the lowest index wins; the key is ``ops.argmax`` of the fused row bit for bit,
    with ``n_offset``; merging into a key that already holds something larger leaves it."""
    ops = ahv.ops
    B, V, N = 3, 3, 4100
    s, Q, A, _ = case(ahv, dev, B, V, N)
    s, Q = np.nan_to_num(s, nan=0.0, posinf=1.0, neginf=-1.0), Q.copy()
    s[:, :, 3000] = s[:, :, 1500] = 7.0
    Q[:, 3000] = Q[:, 1500]
    want, scale, g, margin = vr.fuse(s, Q, A, None, THETA)
    assert margin >= MARGIN
    Qg, Ag, sg = T(Q, dev), T(A, dev), T(s, dev)
    _, slot, counts = ops.view_rotations_compact(Qg, Ag, THETA)
    M = int(counts.max())
    cs = torch.gather(sg, 2, torch.argsort((slot < 0).to(torch.int8), dim=2, stable=True)[:, :, :M])   # participating first, in order
    fd, kd = ops.fuse_view_scores(sg, Qg, Ag, None, THETA, n_offset=1000)
    fc, kc = ops.fuse_view_scores_compact(cs, slot, None, n_offset=1000)
    assert torch.equal(bits(fc), bits(fd)) and torch.equal(kc, kd) and torch.equal(kc, ops.argmax(fc, 1000, return_key=True))
    sc, idx = ops.unpack_best(kc)
    assert torch.equal(bits(fc[:, 1500].contiguous()), bits(fc[:, 3000].contiguous()))
    assert idx.cpu().tolist() == vr.decode(vr.best_keys(fc.cpu().numpy(), 1000))[1].tolist()
    for b in range(B):                              # where the pair of equal rows takes part for some view it wins, at the lower index
        if g[b, :, 1500].any():
            assert idx[b].item() == 2500 and sc[b].item() == 7.0
    big = ops.argmax(torch.full((B, 1), 9.0, device=dev), 77, return_key=True)
    _, merged = ops.fuse_view_scores_compact(cs, slot, None, n_offset=1000, want_scores=False, best_key=big.clone())
    assert torch.equal(merged, big)
    _, reset = ops.fuse_view_scores_compact(cs, slot, None, n_offset=1000, want_scores=False, best_key=big.clone(), reset_best=True)
    assert torch.equal(reset, kc)


# ---- 6. chunks compose and runs repeat -------------------------------------------------------------------------------------

def test_chunks_compose_and_runs_repeat(ahv, dev, head):
    ops = ahv.ops
    B, V, N, CUT, OFF = 3, 3, 4100, 1500, 40
    _, Q, A, _ = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Qg, Ag = T(Q, dev), T(A, dev)
    for w in (None, weights_for(V)):
        kw = dict(weights=w, max_view_angle_deg=THETA, compact=True)
        fused, key = ops.verify_views(refs, query, Qg, Ag, *head, n_offset=OFF, **kw)
        f1, k = ops.verify_views(refs, query, Qg[:, :CUT].contiguous(), Ag, *head, n_offset=OFF, **kw)
        f2, k2 = ops.verify_views(refs, query, Qg[:, CUT:].contiguous(), Ag, *head, n_offset=OFF + CUT, best_key=k, **kw)
        assert k2 is k and torch.equal(k, key)
        assert torch.equal(bits(torch.cat([f1, f2], dim=1)), bits(fused))
        again, key_again = ops.verify_views(refs, query, Qg, Ag, *head, n_offset=OFF, **kw)
        assert torch.equal(bits(again), bits(fused)) and torch.equal(key_again, key)
        first, second = (ops.view_rotations_compact(Qg, Ag, THETA, w) for _ in range(2))
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(bits(first[0]), bits(second[0]))


# ---- 7. captured graph -----------------------------------------------------------------------------------------------------

def test_verify_views_compact_in_a_captured_graph(ahv, dev, head):
    """With ``capacity`` given the step reads nothing on the host: one stream, a linear chain of launches, captured and replayed."""
    ops = ahv.ops
    B, V, N = 3, 3, 1025
    _, Q, A, _ = case(ahv, dev, B, V, N)
    refs, query = volumes(dev, B, V)
    Qg, Ag = T(Q, dev), T(A, dev)
    w = weights_for(V)
    ref, ref_key, counts = ops.verify_views(refs, query, Qg, Ag, *head, weights=w, max_view_angle_deg=THETA, compact=True,
                                            want_counts=True)
    M = max(1, int(counts.max()))
    key = torch.empty(B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused, _, c = ops.verify_views(refs, query, Qg, Ag, *head, weights=w, max_view_angle_deg=THETA, compact=True, capacity=M,
                                       best_key=key, reset_best=True, want_counts=True)
    del w
    for _ in range(2):
        fused.zero_()
        key.zero_()
        c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(fused), bits(ref)) and torch.equal(key, ref_key) and torch.equal(c, counts)


# ---- 8. planted pose -------------------------------------------------------------------------------------------------------

def test_planted_pose_is_found(ahv, dev, head):
    """The construction of tests/test_gpu_views.py::test_planted_pose_is_found under theta = 90 degrees, the reference's own
    threshold: every view is within 90 degrees of the planted pose, and the compact path finds it."""
    ops = ahv.ops
    V, N, PLANT = 4, 4100, 2345
    X = torch.from_numpy(np.random.default_rng(17).standard_normal((1, 16, 8, 8, 8)).astype(np.float32)).to(dev)
    ax = lambda axis, deg: torch.from_numpy(pr_axis(axis, deg)).to(dev)
    A = torch.stack([ax("z", 25.0), ax("x", -30.0) @ ax("y", 20.0), ax("y", 35.0) @ ax("z", -15.0), ax("x", 30.0)])[None]
    Q_true = (ax("y", 15.0) @ ax("x", 10.0))[None]
    Q = T(ahv.rotations.haar_rotations_np(N, seed=23), dev)
    Q[PLANT] = Q_true[0]
    refs = ops.rotate_volume(X.expand(V, -1, -1, -1, -1), A[0])[None]
    query = ops.rotate_volume(X, Q_true)
    fused, key, counts = ops.verify_views(refs, query, Q, A, *head, max_view_angle_deg=90.0, compact=True, want_counts=True)
    score, idx, R_pred = ops.select_rotation(key, Q)
    print("planted pose under 90 degrees: idx %d score %.4f counts %s of %d" % (idx.item(), score.item(), counts.tolist(), N))
    assert idx.item() == PLANT and torch.equal(R_pred, Q_true)
    assert bool((counts < 0.3 * N).all())            # four fifths of the scorer's work is not done
    fd, kd = ops.verify_views(refs, query, Q, A, *head, max_view_angle_deg=90.0)
    assert torch.equal(bits(fused), bits(fd)) and torch.equal(key, kd)
