"""Pose tracking against several posed reference views, CPU tier: argument validation of ``ahv_nearest_views_f32`` /
``ahv_gather_views_f32`` through the ctypes table (validation runs before any HIP call), the host-side checks of the ops, the
numpy reference's own rules (tests/track_views_reference.py), ``track.PoseTracker(views=...)``'s control flow and
``harness.track_sequence(refs=...)`` on an oracle-backed backend, and the full turn with M and the frame count cut to fit."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from . import track_reference as tr
from . import track_views_reference as tvr
from .conftest import REPO


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def _head(g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    return T("W1"), T("W2"), T("b2")


# ---- 1. the entry points refuse bad arguments before any HIP call ---------------------------------------------------
def _refusals(lib, f, ok, prefix):
    def refused(word, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert f(*a) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(prefix) and word in msg, (kw, msg)
    return refused


def test_nearest_views_argument_validation_needs_no_gpu(lib, ahv):
    # (anchor, A, B, V, K, view_idx, A_sel, stream)
    refused = _refusals(lib, lib.ahv_nearest_views_f32, [16, 16, 2, 4, 2, 16, 16, None], b"nearest_views")
    for i in (0, 1, 5, 6):
        refused(b"null", **{"_%d" % i: None})
    refused(b"V =", _3=0)
    refused(b"V =", _3=ahv._lib.AHV_VIEWS_MAX + 1)
    refused(b"K =", _4=0)
    refused(b"K =", _4=5)            # K > V
    refused(b"B =", _2=0)
    refused(b"B >", _2=65536)


def test_gather_views_argument_validation_needs_no_gpu(lib, ahv):
    # (src, view_idx, B, V, K, L, dst, flags, stream)
    refused = _refusals(lib, lib.ahv_gather_views_f32, [16, 16, 2, 3, 2, 8192, 32, 0, None], b"gather_views")
    refused(b"null", _0=None)
    refused(b"null", _6=None)
    refused(b"null", _1=None)        # the indices are needed unless AHV_GATHER_BROADCAST
    refused(b"multiple of 4", _5=8190)
    refused(b"multiple of 4", _5=0)
    refused(b"multiple of 4", _5=-4)
    refused(b"K =", _4=4)            # K > V
    refused(b"V =", _3=17)
    refused(b"B =", _2=0)
    refused(b"aligned", _0=20)
    refused(b"aligned", _6=8)
    refused(b"flags", _7=2)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ahv_nearest_views_f32", "ahv_gather_views_f32"):
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(ahv._lib.SIGNATURES[name][1]), name
    assert ahv._lib.AHV_GATHER_BROADCAST == int(re.search(r"#define AHV_GATHER_BROADCAST (\d+)u", text).group(1))


# ---- 2. the ops check on the host ---------------------------------------------------------------------------------------
def test_ops_check_arguments_before_any_launch(ahv):
    ops = ahv.ops
    A = torch.eye(3).repeat(2, 3, 1, 1)
    anchor = torch.eye(3).repeat(2, 1, 1)
    idx = torch.zeros((2, 2), dtype=torch.int32)
    src = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nearest_views(anchor, A, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_views(src, idx)
    with pytest.raises(RuntimeError, match="outside 1..V"):
        ops.nearest_views(anchor, A, 4)
    with pytest.raises(RuntimeError, match="outside 1..V"):
        ops.nearest_views(anchor, A, 0)
    with pytest.raises(RuntimeError, match="outside 1..V"):
        ops.gather_views(torch.zeros(2, 1, 8), idx)                 # K = 2 > V = 1
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.gather_views(torch.zeros(2, 3, 6), idx)
    with pytest.raises(RuntimeError, match="anchor must be"):
        ops.nearest_views(torch.eye(3), A, 1)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.nearest_views(anchor.clone().requires_grad_(), A, 2)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.gather_views(src.clone().requires_grad_(), idx)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        v = torch.zeros(2, 2, 16, 8, 8, 8)
        ops.verify_views_staged(v.clone().requires_grad_(), v, anchor, A[:, :2], torch.zeros(32, 384), torch.zeros(32, 32),
                                torch.zeros(32))
    with pytest.raises(RuntimeError, match="vol_query must be"):
        v = torch.zeros(2, 2, 16, 8, 8, 8)
        ops.verify_views_staged(v, v[:, :1], anchor, A[:, :2], torch.zeros(32, 384), torch.zeros(32, 32), torch.zeros(32))


# ---- 3. the reference's own rules ------------------------------------------------------------------------------------------
def test_reference_fma_is_correctly_rounded():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((400, 3)).astype(np.float32)
    x[:100, 2] = (-x[:100, 0].astype(np.float64) * x[:100, 1].astype(np.float64)).astype(np.float32)   # cancellation
    x[100:200] *= np.float32(2.0) ** rng.integers(-30, 30, (100, 3)).astype(np.float32)
    for a, b, c in x:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        got = tvr.fma32(a, b, c)
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        d = abs(exact - Fraction(float(got)))
        assert d <= abs(exact - Fraction(float(lo))) and d <= abs(exact - Fraction(float(hi))), (a, b, c)


def test_reference_order_rules():
    nan = np.float32("nan")
    assert tvr.order(np.array([1.0, 3.0, 2.0], np.float32)) == [1, 2, 0]
    assert tvr.order(np.array([2.0, 3.0, 2.0, 3.0], np.float32)) == [1, 3, 0, 2]               # ties: the lower v first
    assert tvr.order(np.array([nan, -5.0, nan, np.float32("-inf")], np.float32)) == [1, 3, 0, 2]   # a NaN behind every number
    assert tvr.order(np.array([0.0, -0.0], np.float32)) == [0, 1]
    src = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    got = tvr.gather_views(src, np.array([[2, 0], [3, -1]]))
    assert np.array_equal(got[0], src[0][[2, 0]]) and not got[1].any()


# ---- 4. PoseTracker(views=...) on the oracle backend ------------------------------------------------------------------------
def _pair(B=2):
    g = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    return torch.from_numpy(g["vol_src"][:B]), torch.from_numpy(g["vol_tgt"][:B])


def _views(ahv, V, seed=11):
    return torch.from_numpy(ahv.rotations.haar_rotations_np(V, seed=seed))


def test_constructor_checks(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    T = ahv.track.PoseTracker
    A = _views(ahv, 3)
    be = lambda: tvr.make_backend(ahv, oracle)
    for kw, word in ((dict(views=A, views_per_step=4), "views_per_step"), (dict(views=A, views_per_step=0), "views_per_step"),
                     (dict(views=A[0]), "views must be"), (dict(views=A[None].repeat(2, 1, 1, 1)), "views must be"),
                     (dict(views=A, max_view_angle_deg=0.0), None), (dict(views_per_step=2), "belong to views"),
                     (dict(max_view_angle_deg=60.0), "belong to views"),
                     (dict(views=torch.eye(3).repeat(17, 1, 1)), "V = 17")):
        with pytest.raises(RuntimeError, match=word):
            T(W1, W2, b2, particles=8, backend=be(), **kw)
    with pytest.raises(RuntimeError, match="symmetry"):
        T(W1, W2, b2, particles=8, backend=be(), views=A, symmetry=object())
    with pytest.raises(RuntimeError, match="nearest_views"):
        T(W1, W2, b2, particles=8, backend=tr.make_backend(ahv, oracle), views=A)       # a backend without the view calls
    t = T(W1, W2, b2, particles=8, backend=be(), views=A)
    assert t.K == t.V == 3 and t.view_selection.idx.dtype == torch.int32                  # views_per_step=None: K = V
    with pytest.raises(RuntimeError, match="init"):
        t.select_views()
    t0 = T(W1, W2, b2, particles=8, backend=be())
    assert t0.view_selection is None
    with pytest.raises(RuntimeError, match="views="):
        t0.select_views()


def test_tracker_control_flow_with_views(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    B, M, N0, V, K, theta = 2, 24, 40, 4, 2, 100.0
    vs, vt = _pair(B)
    refs = torch.from_numpy(np.stack([oracle.rotate_volume(vs.numpy(), ahv.rotations.haar_rotations_np(B, seed=20 + v)) for v in range(V)], 1))
    A = torch.from_numpy(ahv.rotations.haar_rotations_np(B * V, seed=4).reshape(B, V, 3, 3))
    be = tvr.make_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=4.0, n_fresh=3, temperature=0.05, batch=B, seed=3, backend=be,
                              views=A, views_per_step=K, max_view_angle_deg=theta)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    first = t.init(refs, vt, R0)
    assert be.calls == ["verify_views_staged", "select_rotation"]
    # init scores densely over all V views
    sc0, _ = be.verify_views_staged(refs, vt, R0, A, W1, W2, b2, max_view_angle_deg=theta)
    assert torch.equal(sc0, first.scores)
    be.calls.clear()
    assert tuple(first.scores.shape) == (B, N0) and torch.equal(first.idx, first.scores.argmax(dim=1))
    chain = ["track_advance", "resample", "diffuse_rotations", "verify_views_staged", "select_rotation"]
    prev = first
    for n in range(1, 6):
        be.calls.clear()
        with pytest.raises(RuntimeError, match="select_views"):
            t.step()                                                     # nothing selected since the last step
        with pytest.raises(RuntimeError, match="select_views"):
            t.step(refs[:, :K], refs[:, :K], staged=True)
        assert be.calls == []
        want_idx, want_A = tvr.nearest_views(prev.R_map.numpy(), A.numpy(), K)
        if n % 2:   # (B,V,...) inputs: select -> gather -> the chain
            out = t.step(refs, vt)
            assert be.calls == ["nearest_views", "gather_views", "gather_views"] + chain
        else:       # the caller selects, stages and steps
            sel = t.select_views()
            assert sel is t.view_selection and be.calls == ["nearest_views"]
            staged = torch.from_numpy(tvr.gather_views(refs.numpy(), sel.idx.numpy()))
            out = t.step(staged, vt[:, None].expand(B, K, 16, 8, 8, 8).contiguous(), staged=True)
            assert be.calls == ["nearest_views"] + chain
        assert np.array_equal(t.view_selection.idx.numpy(), want_idx) and np.array_equal(t.view_selection.A.numpy(), want_A)
        if n % 2:
            assert np.array_equal(t.buffers[0].numpy(), tvr.gather_views(refs.numpy(), want_idx))
            assert np.array_equal(t.buffers[1].numpy(), tvr.gather_views(vt.numpy(), want_idx, broadcast=True))
        # the step's scores are the K selected views' fused row on the step's particles, and the winner their arg-max
        sc, key = be.verify_views_staged(torch.from_numpy(tvr.gather_views(refs.numpy(), want_idx)), vt, out.particles,
                                         torch.from_numpy(want_A), W1, W2, b2, max_view_angle_deg=theta)
        assert torch.equal(sc, out.scores) and torch.equal(out.idx, torch.nan_to_num(out.scores, nan=float("inf")).argmax(dim=1))
        assert torch.equal(out.particles[:, 0], prev.R_map) and int(t.step_counter[0]) == n
        assert torch.equal(out.R_map, out.particles[torch.arange(B), out.idx])
        prev = out
    with pytest.raises(RuntimeError, match="vol_refs must be"):
        t.step(refs[:, :K], vt)
    with pytest.raises(RuntimeError, match="staged=True belongs"):
        t0 = ahv.track.PoseTracker(W1, W2, b2, particles=8, batch=B, backend=tr.make_backend(ahv, oracle))
        t0.init(vs, vt, R0)
        t0.step(vs, vt, staged=True)


def test_one_identity_view_is_the_single_reference_tracker(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(1)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(16, seed=5))

    def run(views, seed=1):
        be = tvr.make_backend(ahv, oracle)
        kw = dict(views=torch.eye(3)[None]) if views else {}
        t = ahv.track.PoseTracker(W1, W2, b2, particles=16, n_fresh=2, batch=1, seed=seed, backend=be, **kw)
        out = [t.init(vs[:, None] if views else vs, vt, R0)]
        out += [t.step(vs[:, None] if views else vs, vt) for _ in range(3)]
        return [(o.particles.clone(), o.scores.clone(), o.R_map.clone(), o.idx.clone()) for o in out]

    a, b, c, d = run(False), run(True), run(True), run(True, seed=2)
    for x, y, z in zip(a, b, c):
        assert all(torch.equal(p, q) and torch.equal(q, r) for p, q, r in zip(x, y, z))
    assert not torch.equal(c[1][0], d[1][0])


# ---- 5. track_sequence(refs=...) -------------------------------------------------------------------------------------------
def test_track_sequence_with_reference_views(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    item = list(ahv.harness.SyntheticSequences(n_seq=1, n_frames=7, seed=3))[0]
    vols, batches = {}, []

    class Model:
        """Stands in for the encoder: a fixed random volume per (reference, frame) pair (what is under test is the plumbing)."""

        def forward_features(self, a, b):
            batches.append((len(a), len(b)))
            key = lambda x: float(x.flatten()[0])
            f = lambda k: vols.setdefault(k, torch.randn(16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return (torch.stack([f(("ref", key(x))) for x in a]), torch.stack([f((key(x), key(y))) for x, y in zip(a, b)]))

    refs = [5, 0, 2]
    props = torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9))
    mk = lambda **kw: ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=tvr.make_backend(ahv, oracle),
                                            views=item["R"][refs], **kw)
    t = mk(views_per_step=2, max_view_angle_deg=170.0)
    res = ahv.harness.track_sequence(Model(), item, t, refs=refs, views_per_step=2, max_view_angle_deg=170.0, proposals=props,
                                     device="cpu")
    order = [1, 3, 4, 6]
    assert res["frames"] == order and batches == [(3, 3), (2, 2), (2, 2), (2, 2)]      # V pairs for init, then K per frame
    assert tuple(res["R_map"].shape) == (4, 3, 3) and int(t.step_counter[0]) == 3
    for k, f in enumerate(order):   # the error is taken against the frame's absolute rotation
        assert abs(float(res["err"][k]) - float(ahv.rotations.geodesic_deg(res["R_map"][k][None], item["R"][f][None]))) < 1e-4
    assert t.ops.calls.count("nearest_views") == 3 and t.ops.calls.count("gather_views") == 3
    for kw, word in ((dict(refs=[0, 0, 2]), "distinct"), (dict(refs=[0, 1]), "distinct"), (dict(refs=refs, views_per_step=3), "built with"),
                     (dict(refs=refs, max_view_angle_deg=60.0), "built with")):
        with pytest.raises(RuntimeError, match=word):
            ahv.harness.track_sequence(Model(), item, mk(views_per_step=2, max_view_angle_deg=170.0), proposals=props, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="belong to refs"):
        ahv.harness.track_sequence(Model(), item, t, views_per_step=2, device="cpu")
    with pytest.raises(RuntimeError, match="views="):
        ahv.harness.track_sequence(Model(), item, ahv.track.PoseTracker(W1, W2, b2, particles=4, batch=1), refs=refs, device="cpu")


def test_track_sequence_with_reference_views_and_row_vector_annotations(ahv, oracle, g128):
    """``row_vector_R=True``: a model of the row-vector convention gives the pair (src, tgt) the rotation ``R_src^T R_tgt``.  The
    stand-in encoder is such a model, exactly: the volume of frame k is ``rotate_volume(X, R_k)``, and ``rotate_volume(vol_s, M)``
    samples X at ``R_s M x``, so it equals ``vol_t`` at ``M = R_s^T R_t`` for ANY rotations.  The harness encodes (frame,
    reference), whose rotation ``R_t^T R_v`` is ``Q A_v^T`` with ``Q = R_t^T`` and ``A_v = R_v^T``: every view's maximum is at
    ``R_t^T``.  The first tracked frame's ``R_t^T`` is among the proposals (its score is the maximum, 1), the truth then moves 3
    degrees per frame about a generic axis and the particles diffuse by sigma = 3 degrees: the bar is 2 sigma = 6 degrees on
    every frame.  Measured on the oracle backend: largest error 2.87 degrees."""
    W1, W2, b2 = _head(g128)
    n, refs = 9, [0, 4, 8]
    X = tvr.turn_volume()
    base = ahv.rotations.haar_rotations_np(1, seed=21)[0].astype(np.float64)
    axis = np.array([0.3, 0.5, -0.81])
    R = (base[None] @ tr.exp_so3(np.arange(n)[:, None] * np.radians(3.0) * (axis / np.linalg.norm(axis))[None])).astype(np.float32)
    item = {"n": n, "model_id": "row_plant", "R": torch.from_numpy(R),
            "layer4": torch.arange(n, dtype=torch.float32)[:, None, None, None].expand(n, 4, 2, 2).contiguous()}   # the frame's number
    seen = []

    class Model:
        def forward_features(self, a, b):
            ids = lambda x: [int(v) for v in x[:, 0, 0, 0]]
            seen.append((ids(a), ids(b)))
            vol = lambda k: torch.from_numpy(oracle.rotate_volume(X, R[k][None]))[0]
            return torch.stack([vol(k) for k in ids(a)]), torch.stack([vol(k) for k in ids(b)])

    order = [1, 2, 3, 5, 6, 7]
    props = torch.from_numpy(np.concatenate([ahv.rotations.haar_rotations_np(255, seed=9), R[1].T[None]]))
    t = ahv.track.PoseTracker(W1, W2, b2, particles=64, sigma_deg=3.0, temperature=0.02, batch=1, seed=1,
                              backend=tvr.make_backend(ahv, oracle), views=item["R"][refs].transpose(-1, -2), views_per_step=2,
                              max_view_angle_deg=60.0)
    res = ahv.harness.track_sequence(Model(), item, t, refs=refs, row_vector_R=True, proposals=props, device="cpu")
    assert res["frames"] == order
    assert seen[0] == ([1, 1, 1], refs)                                  # (frame, reference): the frame's volume is rotated
    assert all(a == [f, f] and set(b) <= set(refs) and len(set(b)) == 2 for (a, b), f in zip(seen[1:], order[1:]))
    for k, f in enumerate(order):   # the pose is R_t^T, and the error is taken against it
        assert abs(float(res["err"][k]) - float(ahv.rotations.geodesic_deg(res["R_map"][k][None], item["R"][f].T[None]))) < 1e-4
    print("row-vector plant: err %s" % " ".join("%.2f" % e for e in res["err"].tolist()))
    assert float(res["err"][0]) < 1e-3 and float(res["err"].max()) < 6.0


# ---- 6. the full turn, cut to fit the CPU ------------------------------------------------------------------------------------
def test_full_turn_cut_to_fit(ahv, oracle, g128):
    """The plant of tests/track_views_reference.py with 256 particles over frames 0-36 (108 degrees: the selection changes at
    22.5 and 67.5 degrees), the blind fused arg-max over all 8 views on frames 0, 12, 24, 36 (only the pairs inside the angle are
    scored: the others never enter a sum).  Measured on the oracle backend with numpy noise: tracker max over frames 6-36
    3.16 degrees, blind median 8.15 degrees (4.8, 14.1, 6.1, 10.2)."""
    P = tvr.TURN
    W1, W2, b2 = _head(g128)
    frames, M = 37, 256
    X = tvr.turn_volume()
    A = tvr.turn_views()
    rot = lambda R: oracle.rotate_volume(X, np.asarray(R, np.float32).reshape(1, 3, 3))
    refs = torch.from_numpy(np.stack([rot(a)[0] for a in A])[None])                     # (1,V,16,8,8,8)
    truth = tvr.turn_truth(frames)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(P["n_init"], seed=P["init_seed"]))
    be = tvr.make_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"], temperature=P["temperature"],
                              batch=1, seed=0, backend=be, views=torch.from_numpy(A), views_per_step=P["views_per_step"],
                              max_view_angle_deg=P["max_view_angle_deg"])
    track, blind, picked = [], [], []
    for k in range(frames):
        q = torch.from_numpy(rot(truth[k]))
        res = t.init(refs, q, R0) if k == 0 else t.step(refs, q)
        track.append(float(tr.geodesic_deg(res.R_map[0].double().numpy(), truth[k])))
        if k:
            picked.append(tuple(sorted(t.view_selection.idx[0].tolist())))
        if k % P["blind_every"] == 0:
            _, key = be.verify_views_staged(refs, q, R0, torch.from_numpy(A)[None], W1, W2, b2, max_view_angle_deg=P["max_view_angle_deg"])
            blind.append(float(tr.geodesic_deg(R0.numpy()[int(ahv.dist.unpack_keys_host(key.numpy())[1][0])], truth[k])))
    worst, median = tvr.turn_bar(track, blind)
    print("full turn (cut): tracker %s | max from frame 6 %.3f | blind %s | blind median %.3f | selections %s"
          % (" ".join("%.2f" % e for e in track), worst, " ".join("%.1f" % e for e in blind), median, sorted(set(picked))))
    assert len(set(picked)) >= 3          # the selection moved along the turn
    assert worst < median
