"""Pose tracking against several posed reference views, on the device: ``ahv_nearest_views_f32`` / ``ahv_gather_views_f32`` against
the numpy reference and ``torch.gather`` (exact equality everywhere), ``ops.verify_views_staged`` against the calls it is made
of, ``track.PoseTracker(views=...)`` (one identity view against the single-reference tracker, determinism, the captured step
across a change of selection, the smoothers) and the full turn.

Figures measured on the MI355X (this file prints them; DESIGN 4.2 quotes them):
  full turn, tracker max over frames 6-119 / blind fused arg-max median over frames 0, 12, ..., 108: 3.38 / 7.20 degrees
"""
import math

import numpy as np
import pytest
import torch

from . import track_reference as tr
from . import track_views_reference as tvr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
VOL = (16, 8, 8, 8)


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


def _views(ahv, B, V, seed):
    return ahv.rotations.haar_rotations_np(B * V, seed=seed).reshape(B, V, 3, 3)


# ---- 1. nearest_views against the reference ------------------------------------------------------------------------------
def _check_nearest(ops, dev, anchor, A, K):
    sel = ops.nearest_views(_t(anchor).to(dev), _t(A).to(dev), K)
    idx, A_sel = tvr.nearest_views(anchor, A, K)
    assert sel.idx.dtype == torch.int32 and np.array_equal(sel.idx.cpu().numpy(), idx), (A.shape, K)
    assert _bytes_equal(sel.A.cpu(), _t(A_sel)), (A.shape, K)                                   # bit copies of A[idx]
    rows = _t(A)[torch.arange(len(A))[:, None], sel.idx.cpu().long()]
    assert _bytes_equal(sel.A.cpu(), rows)
    return sel


@pytest.mark.parametrize("B", [1, 3])
def test_nearest_views_matches_the_reference(ahv, ops, dev, B):
    for V in (1, 2, 16):
        A = _views(ahv, B, V, seed=30 + V)
        anchor = ahv.rotations.haar_rotations_np(B, seed=7 + V)
        for K in sorted({1, min(2, V), V}):
            _check_nearest(ops, dev, anchor, A, K)
    # more samples than one workgroup serves (16), with a ragged end
    A, anchor = _views(ahv, 37, 5, seed=3), ahv.rotations.haar_rotations_np(37, seed=4)
    _check_nearest(ops, dev, anchor, A, 3)


def test_nearest_views_ties_nans_and_any_anchor(ahv, ops, dev):
    B, V = 3, 16
    A = _views(ahv, B, V, seed=41)
    anchor = ahv.rotations.haar_rotations_np(B, seed=42)
    # two identical views: the lower v comes first (make the pair the nearest of all: a copy of the anchor itself)
    tie = A.copy()
    tie[:, 9] = anchor
    tie[:, 4] = anchor
    for K in (1, 2, V):
        sel = _check_nearest(ops, dev, anchor, tie, K)
        assert (sel.idx[:, 0] == 4).all() and (K == 1 or (sel.idx[:, 1] == 9).all())
    same = np.broadcast_to(A[:, :1], A.shape).copy()                       # every view the same: the order is v
    sel = _check_nearest(ops, dev, anchor, same, V)
    assert torch.equal(sel.idx.cpu(), torch.arange(V, dtype=torch.int32).expand(B, V))
    # a NaN view matrix ranks last, NaNs among themselves by v; its matrix is copied with its bits
    bad = A.copy()
    bad[0, 3] = np.nan
    bad[1, 0, 1, 1] = np.nan
    bad[2, 5] = np.nan
    bad[2, 2, 0, 0] = np.nan
    sel = _check_nearest(ops, dev, anchor, bad, V)
    assert sel.idx[0, -1] == 3 and sel.idx[1, -1] == 0 and sel.idx[2, -2:].tolist() == [2, 5]
    _check_nearest(ops, dev, anchor, bad, 2)
    # an anchor that is no rotation (and one with a NaN: every t is NaN, the order is v)
    rng = np.random.default_rng(5)
    wild = (rng.standard_normal((B, 3, 3)) * np.array([1e-3, 1.0, 1e4])[:, None, None]).astype(np.float32)
    for K in (1, 5, V):
        _check_nearest(ops, dev, wild, A, K)
    wild[1, 2, 2] = np.nan
    sel = _check_nearest(ops, dev, wild, A, V)
    assert sel.idx[1].tolist() == list(range(V))
    # out=: written in place
    out = ops.ViewSelection(torch.full((B, 2), -7, dtype=torch.int32, device=dev), torch.zeros((B, 2, 3, 3), device=dev))
    got = ops.nearest_views(_t(anchor).to(dev), _t(A).to(dev), 2, out=out)
    assert got is out and np.array_equal(out.idx.cpu().numpy(), tvr.nearest_views(anchor, A, 2)[0])


@pytest.mark.parametrize("V,K", [(16, 2), (4, 1), (8, 7)])
def test_selection_agrees_with_participation(ahv, ops, dev, V, K):
    """Under an angle limit placed between the K-th and the (K+1)-th trace, the views ``fuse_view_scores`` lets take part in the
    anchor are exactly the K selected (one fused call per view, every other weight 0: -inf where that view does not take part)."""
    B = 3
    A = _views(ahv, B, V, seed=50 + V)
    anchor = ahv.rotations.haar_rotations_np(B, seed=60 + V)
    t = np.sort(tvr.traces(anchor, A).astype(np.float64), axis=1)[:, ::-1]
    Ad, Qd = _t(A).to(dev), _t(anchor[:, None]).to(dev)                   # the anchor as the one hypothesis per sample
    sel = ops.nearest_views(_t(anchor).to(dev), Ad, K)
    for b in range(B):                                                      # (the limit is one angle per call)
        lo, hi = t[b, K], t[b, K - 1]
        assert hi - lo > 1e-4 and -1.0 < lo and hi < 3.0, "the fixture's traces must leave room for a limit"
        theta = math.degrees(math.acos((0.5 * (lo + hi) - 1.0) / 2.0))
        took = []
        for v in range(V):
            w = [1.0 if u == v else 0.0 for u in range(V)]
            fused, _ = ops.fuse_view_scores(torch.ones((B, V, 1), device=dev), Qd, Ad, weights=w, max_view_angle_deg=theta)
            if float(fused[b, 0]) == 1.0:
                took.append(v)
            else:
                assert float(fused[b, 0]) == -math.inf
        assert sorted(sel.idx[b].tolist()) == took, (b, theta)


# ---- 2. gather_views against torch.gather ------------------------------------------------------------------------------------
def _any_bits(shape, seed, dev):
    """float32 tensors of arbitrary bit patterns (NaN payloads, denormals, infinities included)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(1 << 31), (1 << 31) - 1, shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).to(dev)


@pytest.mark.parametrize("L", [4, 8192, 8196])
def test_gather_views_is_torch_gather(ops, dev, L):
    B, V, K = 2, 3, 2
    src = _any_bits((B, V, L), L, dev)
    for rows in ([[2, 0], [1, 1]], [[0, 1], [2, 0]]):
        idx = torch.tensor(rows, dtype=torch.int32, device=dev)
        want = torch.gather(_bits(src), 1, idx.long()[:, :, None].expand(B, K, L))
        assert torch.equal(_bits(ops.gather_views(src, idx)), want)
    # broadcast: src has no view axis, every k receives src[b]
    one = _any_bits((B, L), L + 1, dev)
    got = ops.gather_views(one, idx, broadcast=True)
    assert tuple(got.shape) == (B, K, L) and torch.equal(_bits(got), _bits(one)[:, None].expand(B, K, L))
    # an index outside 0..V-1 gives a row of zeros and touches nothing else: guard bands around dst stay as they were
    guard = 64
    buf = torch.full((guard + B * K * L + guard,), 7.5, device=dev)
    dst = buf[guard:guard + B * K * L].view(B, K, L)
    idx = torch.tensor([[3, 1], [-1, 2]], dtype=torch.int32, device=dev)
    assert ops.gather_views(src, idx, out=dst) is dst
    assert not _bits(dst[0, 0]).any() and not _bits(dst[1, 0]).any()
    assert torch.equal(_bits(dst[0, 1]), _bits(src[0, 1])) and torch.equal(_bits(dst[1, 1]), _bits(src[1, 2]))
    assert (buf[:guard] == 7.5).all() and (buf[-guard:] == 7.5).all()
    if L == 8192:     # trailing dimensions of any shape: a feature volume
        vol = src.view((B, V) + VOL)
        assert torch.equal(_bits(ops.gather_views(vol, idx)), _bits(dst).view((B, K) + VOL))


def test_refusals(ops, dev):
    B, V, K = 2, 3, 2
    idx = torch.zeros((B, K), dtype=torch.int32, device=dev)
    src = torch.zeros((B, V, 8), device=dev)
    A = torch.eye(3, device=dev).repeat(B, V, 1, 1)
    anchor = torch.eye(3, device=dev).repeat(B, 1, 1)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.gather_views(torch.zeros((B, V, 6), device=dev), idx)
    with pytest.raises(RuntimeError, match="outside 1..V"):
        ops.gather_views(src[:, :1].contiguous(), idx)                     # K > V
    with pytest.raises(RuntimeError, match="outside 1..V"):
        ops.nearest_views(anchor, A, V + 1)
    base = torch.zeros((B * V * 8 + 4,), device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.gather_views(base[1:1 + B * V * 8].view(B, V, 8), idx)         # src 4 bytes off
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.gather_views(src, idx, out=base[2:2 + B * K * 8].view(B, K, 8))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gather_views(torch.zeros((B, V, 16), device=dev)[:, :, ::2], idx)
    with pytest.raises(RuntimeError, match="int32"):
        ops.gather_views(src, idx.long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_views(src.cpu(), idx.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nearest_views(anchor.cpu(), A.cpu(), K)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.gather_views(src.clone().requires_grad_(), idx)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.nearest_views(anchor, A.clone().requires_grad_(), K)
    # the library refuses the same before any launch
    lib = ops._lib.load()
    assert lib.ahv_gather_views_f32(src.data_ptr(), idx.data_ptr(), B, V, K, 6, src.data_ptr(), 0, None) == -1
    assert b"multiple of 4" in lib.ahv_last_error()
    assert lib.ahv_gather_views_f32(src.data_ptr() + 4, idx.data_ptr(), B, V, K, 8, src.data_ptr(), 0, None) == -1
    assert b"aligned" in lib.ahv_last_error()
    assert lib.ahv_nearest_views_f32(anchor.data_ptr(), A.data_ptr(), B, V, V + 1, idx.data_ptr(), A.data_ptr(), None) == -1
    assert b"K =" in lib.ahv_last_error()


# ---- 3. verify_views_staged is the calls it is made of ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(ahv, dev):
    """B = 2, V = 4, K = 2, N = 130 (more than one tile of the scorer's lanes, a ragged end)."""
    B, V, N = 2, 4, 130
    g = torch.Generator().manual_seed(3)
    refs = torch.randn((B, V) + VOL, generator=g).to(dev)
    query = torch.randn((B,) + VOL, generator=g).to(dev)
    query_v = torch.randn((B, V) + VOL, generator=g).to(dev)
    A = _t(_views(ahv, B, V, seed=8)).to(dev)
    Q = _t(ahv.rotations.haar_rotations_np(B * N, seed=9).reshape(B, N, 3, 3)).to(dev)
    return refs, query, query_v, A, Q


@pytest.mark.parametrize("theta", [None, 100.0])
def test_staged_with_a_shared_query_is_verify_views(ops, dev, head, scene, theta):
    refs, query, _, A, Q = scene
    B, V, N, K = 2, 4, 130, 2
    sel = ops.nearest_views(Q[:, 0].contiguous(), A, K)
    refs_k = ops.gather_views(refs, sel.idx)
    pick = sel.idx.long()
    assert _bytes_equal(refs_k, refs[torch.arange(B)[:, None], pick]) and _bytes_equal(sel.A, A[torch.arange(B)[:, None], pick])
    want_s, want_k = ops.verify_views(refs_k, query, Q, sel.A, *head, max_view_angle_deg=theta)
    got_s, got_k = ops.verify_views_staged(refs_k, query, Q, sel.A, *head, max_view_angle_deg=theta)
    assert _bytes_equal(got_s, want_s) and torch.equal(got_k, want_k)
    if theta is not None:
        assert torch.isinf(want_s).any() and torch.isfinite(want_s).any()      # the limit bites, and not everywhere
    # with the caller's buffers: the same bytes, merged into the key unless reset, and no allocation
    ws = ops.verify_views_workspace(B, K, N, dev)
    s_out = torch.empty((B, N), device=dev)
    key = torch.full((B,), (1 << 62), dtype=torch.int64, device=dev)
    ops.verify_views_staged(refs_k, query, Q, sel.A, *head, max_view_angle_deg=theta, workspace=ws, scores_out=s_out, best_key=key)
    assert (key == (1 << 62)).all()                                              # merged: the larger key stays
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    r = ops.verify_views_staged(refs_k, query, Q, sel.A, *head, max_view_angle_deg=theta, workspace=ws, scores_out=s_out,
                                best_key=key, reset_best=True)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    assert r[0] is s_out and r[1] is key and _bytes_equal(s_out, want_s) and torch.equal(key, want_k)
    # hypotheses shared by the batch
    want = ops.verify_views(refs_k, query, Q[0], sel.A, *head, max_view_angle_deg=theta)
    got = ops.verify_views_staged(refs_k, query, Q[0], sel.A, *head, max_view_angle_deg=theta)
    assert _bytes_equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(RuntimeError, match="workspace was made for"):
        ops.verify_views_staged(refs_k, query, Q[:, :100].contiguous(), sel.A, *head, workspace=ws)


def test_staged_with_a_query_per_view_is_verify_pair_then_fuse(ops, dev, head, scene):
    refs, _, query_v, A, Q = scene
    B, V, N, K, theta = 2, 4, 130, 2, 100.0
    sel = ops.nearest_views(Q[:, 0].contiguous(), A, K)
    refs_k, query_k = ops.gather_views(refs, sel.idx), ops.gather_views(query_v, sel.idx)
    Rv = ops.view_rotations(Q, sel.A).reshape(B * K, N, 3, 3)
    per_view, _ = ops.verify_pair(refs_k.reshape((B * K,) + VOL), query_k.reshape((B * K,) + VOL), Rv, *head)
    want_s, want_k = ops.fuse_view_scores(per_view.reshape(B, K, N), Q, sel.A, max_view_angle_deg=theta)
    got_s, got_k = ops.verify_views_staged(refs_k, query_k, Q, sel.A, *head, max_view_angle_deg=theta)
    assert _bytes_equal(got_s, want_s) and torch.equal(got_k, want_k)
    shared = ops.verify_views_staged(refs_k, query_k[:, 0].contiguous(), Q, sel.A, *head, max_view_angle_deg=theta)[0]
    assert not _bytes_equal(shared, got_s)                                        # the per-view queries were read


# ---- 4. PoseTracker(views=...) ----------------------------------------------------------------------------------------------------
def _copy(o):
    return type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o])


FIELDS = ("particles", "scores", "score", "idx", "R_map", "reacquired")


def _same(x, y, draws=True):
    for name in FIELDS:
        assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), name
    if draws and x.draws is not None:
        assert torch.equal(x.draws, y.draws)


def test_one_identity_view_is_the_single_reference_tracker(ahv, ops, dev, head):
    g = load_golden("batched")
    vs, vt = _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev)
    B = vs.shape[0]
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    frames = [(0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous() for k in range(4)]

    def run(views, seed=1, **kw):
        if views:
            kw.update(views=torch.eye(3, device=dev)[None])
        t = ahv.track.PoseTracker(*head, particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=seed, **kw)
        src = vs[:, None].contiguous() if views else vs
        return [_copy(t.init(src, vt, R0))] + [_copy(t.step(src, f)) for f in frames]

    single, views, again, other = run(False), run(True), run(True), run(True, seed=2)
    for x, y, z in zip(single, views, again):
        _same(x, y)                                    # V = K = 1, A = I: byte-identical to the single-reference tracker
        _same(y, z)                                    # the same seed gives the same bytes
    assert not torch.equal(views[1].particles, other[1].particles)
    # history and marginals observe and never steer
    smooth = run(True, history=4, marginals=True)
    for x, y in zip(views, smooth):
        _same(x, y)


def _turn(ahv, ops, dev, frames, start_deg, deg_per_frame):
    """The plant of tests/track_views_reference.py on the device: (refs (1,V,...), queries (frames,...), A (V,3,3), truth)."""
    X = _t(tvr.turn_volume()).to(dev)
    A = tvr.turn_views()
    t = np.arange(frames, dtype=np.float64)[:, None]
    truth = tr.exp_so3((math.radians(start_deg) + t * math.radians(deg_per_frame)) * tvr.turn_axis()[None])
    refs = ops.rotate_volume(X.expand((len(A),) + VOL), _t(A).to(dev))[None].contiguous()
    queries = ops.rotate_volume(X.expand((frames,) + VOL), _t(truth.astype(np.float32)).to(dev))
    return refs, queries, A, truth


def test_captured_steps_equal_eager_steps_across_a_change_of_selection(ahv, ops, dev, head):
    """6 steps, M = 64, V = 4 of the plant's views, K = 2, 5 degrees per frame from 30 to 60 degrees: the two nearest views are
    {0, 1} before 45 degrees and {1, 2} after, so the replayed graphs (captured by steps 2 and 3, at 40 and 45 degrees) must
    follow a selection that changed after they were captured."""
    steps = 6
    refs, queries, A, _ = _turn(ahv, ops, dev, steps + 1, 30.0, 5.0)
    refs, A = refs[:, :4].contiguous(), A[:4]
    R0 = _t(ahv.rotations.haar_rotations_np(4096, seed=5)).to(dev)

    def run(mode, **kw):
        t = ahv.track.PoseTracker(*head, particles=64, sigma_deg=4.0, n_fresh=4, temperature=0.02, batch=1, seed=3,
                                  views=_t(A).to(dev), views_per_step=2, max_view_angle_deg=60.0, **kw)
        outs, picks = [_copy(t.init(refs, queries[:1], R0))], []
        with pytest.raises(RuntimeError, match="select_views"):
            t.step()
        for k in range(1, steps + 1):
            if mode == "full":
                o = t.step(refs, queries[k:k + 1])
            else:   # the caller selects and stages, then steps on the buffers
                sel = t.select_views()
                staged = (ops.gather_views(refs, sel.idx), ops.gather_views(queries[k:k + 1], sel.idx, broadcast=True))
                if mode == "staged":
                    o = t.step(*staged, staged=True)
                else:
                    t.buffers[0].copy_(staged[0])
                    t.buffers[1].copy_(staged[1])
                    o = t.step()
            outs.append(_copy(o))
            picks.append(tuple(t.view_selection.idx[0].tolist()))
        return outs, picks, t

    eager, picks, _ = run("full")
    assert set(picks[1]) == {0, 1} and set(picks[-1]) == {1, 2}, picks      # the selection changed after the captures
    for mode, kw in (("full", dict(use_graph=True)), ("staged", {}), ("staged", dict(use_graph=True)), ("buffers", dict(use_graph=True)),
                     ("full", dict(history=4, marginals=True)), ("full", dict(history=4, marginals=True, use_graph=True))):
        got, got_picks, t = run(mode, **kw)
        assert got_picks == picks, (mode, kw)
        for k, (x, y) in enumerate(zip(eager, got)):
            _same(x, y)                                # (the smoothers observe and never steer)
        if kw.get("use_graph"):
            assert sorted(t._graphs) == [(0, mode != "full"), (1, mode != "full")]
        if kw.get("history"):
            path, marg = t.smoothed(), t.smoothed_marginals()
            assert tuple(path.R.shape) == (1, 4, 3, 3) and tuple(marg.logw.shape) == (1, 4, 64)
            assert torch.isfinite(path.R).all() and not torch.isnan(marg.logw).any()


def test_full_turn_on_the_device(ahv, ops, dev, head):
    """The plant of tests/track_views_reference.py: 8 views 45 degrees apart, K = 2, 60 degrees, 512 particles, 120 frames of 3
    degrees (a full turn).  Bar: the tracker's largest error over frames 6-119 stays below the median error of the blind fused
    arg-max (``ops.verify_views`` over all 8 views on the 4 096 hypotheses of ``init``) on frames 0, 12, ..., 108.
    Measured on the MI355X: tracker max 3.38 degrees (median 1.24), blind median 7.20 degrees."""
    P = tvr.TURN
    refs, queries, A, truth = _turn(ahv, ops, dev, P["frames"], 0.0, P["deg_per_frame"])
    Ad = _t(A).to(dev)
    R0 = _t(ahv.rotations.haar_rotations_np(P["n_init"], seed=P["init_seed"])).to(dev)
    t = ahv.track.PoseTracker(*head, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                              temperature=P["temperature"], batch=1, seed=0, views=Ad, views_per_step=P["views_per_step"],
                              max_view_angle_deg=P["max_view_angle_deg"])
    R_map, blind, picks = [], [], []
    for k in range(P["frames"]):
        q = queries[k:k + 1]
        res = t.init(refs, q, R0) if k == 0 else t.step(refs, q)
        R_map.append(res.R_map[0].clone())
        picks.append(t.view_selection.idx[0].clone())
        if k % P["blind_every"] == 0:
            _, key = ops.verify_views(refs, q, R0, Ad[None], *head, max_view_angle_deg=P["max_view_angle_deg"], want_scores=False)
            blind.append(ops.select_rotation(key, R0)[2][0])
    R_map, blind = torch.stack(R_map).double().cpu().numpy(), torch.stack(blind).double().cpu().numpy()   # the one host copy
    track = tr.geodesic_deg(R_map, truth)
    blind_err = tr.geodesic_deg(blind, truth[::P["blind_every"]])
    worst, median = tvr.turn_bar(track, blind_err)
    seen = sorted({tuple(sorted(p.tolist())) for p in picks[1:]})
    print("full turn on the device: tracker max from frame 6 %.3f (median %.3f) | blind %s | blind median %.3f | selections %s"
          % (worst, float(np.median(track[P["late"]:])), " ".join("%.1f" % e for e in blind_err), median, seen))
    assert len(blind_err) == 10 and len(seen) >= 8      # the selection went round with the object
    assert worst < median
