"""Trajectory smoothing, CPU tier: argument validation of ``ahv_smooth_step_f32`` / ``ahv_smooth_backtrace_f32`` through the
ctypes table (validation runs before any HIP call), the host-side checks of the ops and of ``track.PoseTracker(history=H)``,
the fp64 reference (tests/smooth_reference.py) against a brute-force path maximiser, the backtrace's break rule, the control
flow of the tracker on an oracle-backed backend, and the planted sequence with two distractor frames."""
import math
import os
import re

import numpy as np
import pytest
import torch

from . import smooth_reference as sm
from . import track_cv_reference as cv
from . import track_reference as tr
from .conftest import REPO

INF = float("inf")
WALK_CALLS = ["track_advance", "resample", "diffuse_rotations", "verify_pair", "select_rotation"]
CV_CALLS = ["track_advance", "resample", "predict_rotations", "verify_pair", "select_rotation"]


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def _head(g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    return T("W1"), T("W2"), T("b2")


def _pair(B=2):
    g = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    return torch.from_numpy(g["vol_src"][:B]), torch.from_numpy(g["vol_tgt"][:B])


# ---- 1. the entry points refuse bad arguments before any HIP call ------------------------------------------------------
def _refuser(lib, f, ok, prefix):
    def refused(word, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert f(*a) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(prefix) and word in msg, (kw, msg)
    return refused


def test_smooth_step_argument_validation_needs_no_gpu(lib):
    # (0 R_cur, 1 scores, 2 V_cur, 3 step, 4 first_step, 5 B, 6 M, 7 H, 8 beta, 9 sigma, 10 jump, 11 damping, 12 hist_R, 13 hist_P,
    #  14 hist_delta, 15 hist_back, 16 stream)
    ok = [1, 1, None, 1, 1, 2, 8, 4, 50.0, 0.05, 8.0, 1.0, 1, None, 1, 1, None]
    refused = _refuser(lib, lib.ahv_smooth_step_f32, ok, b"smooth_step")
    for slot in (0, 1, 3, 12, 14, 15):
        refused(b"null", **{"_%d" % slot: None})
    refused(b"both or neither", _2=1)
    refused(b"both or neither", _13=1)
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _6=bad)
    for bad in (0, -1, 65536):
        refused(b"B =", _5=bad)
    for bad in (1, 0, -2, 1 << 31):
        refused(b"H =", _7=bad)
    for bad in (0.0, -1.0, INF, float("nan")):
        refused(b"beta", _8=bad)
    for bad in (0.0, -0.1, INF, float("nan"), 1e-20):
        refused(b"sigma", _9=bad)
    for bad in (-0.5, float("nan"), -INF):
        refused(b"jump", _10=bad)
    for bad in (-0.01, 1.01, INF, float("nan")):
        refused(b"damping", _11=bad)


def test_smooth_backtrace_argument_validation_needs_no_gpu(lib):
    # (0 hist_R, 1 hist_delta, 2 hist_back, 3 step, 4 first_step, 5 B, 6 M, 7 H, 8 F, 9 path_idx, 10 path_R, 11 stream)
    ok = [1, 1, 1, 1, 1, 2, 8, 4, 4, 1, 1, None]
    refused = _refuser(lib, lib.ahv_smooth_backtrace_f32, ok, b"smooth_backtrace")
    for slot in (0, 1, 2, 3, 9, 10):
        refused(b"null", **{"_%d" % slot: None})
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _6=bad)
    for bad in (0, 65536):
        refused(b"B =", _5=bad)
    for bad in (1, 0, 1 << 31):
        refused(b"H =", _7=bad)
    for bad in (0, -1, 5):
        refused(b"F =", _8=bad)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n in (("ahv_smooth_step_f32", 17), ("ahv_smooth_backtrace_f32", 12)):
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        args = [a.strip() for a in proto.split(",")]
        sig = ahv._lib.SIGNATURES[name][1]
        assert len(args) == len(sig) == n
        for a, c in zip(args, sig):      # pointer <-> void*, int64_t <-> c_int64, int <-> c_int, float <-> c_float
            kind = ("p" if "*" in a else "i64" if a.startswith("int64_t") else "int" if a.startswith("int") else "f")
            assert kind == {"c_void_p": "p", "c_long": "i64", "c_int": "int", "c_float": "f"}[c.__name__], (name, a, c)


# ---- 2. the ops check on the host ------------------------------------------------------------------------------------
def test_ops_check_arguments_before_any_launch(ahv):
    ops = ahv.ops
    for bad in (1, 0, -1):
        with pytest.raises(RuntimeError, match="H ="):
            ops.smooth_history(2, 8, bad, "cpu")
    with pytest.raises(RuntimeError, match="B ="):
        ops.smooth_history(0, 8, 4, "cpu")
    with pytest.raises(RuntimeError, match="M ="):
        ops.smooth_history(2, 0, 4, "cpu")
    h = ops.smooth_history(2, 8, 4, "cpu")
    assert tuple(h.R.shape) == (4, 2, 8, 3, 3) and h.P is None and tuple(h.delta.shape) == (4, 2, 8)
    assert h.back.dtype == torch.int32 and tuple(h.back.shape) == (4, 2, 8)
    assert tuple(ops.smooth_history(2, 8, 4, "cpu", velocities=True).P.shape) == (4, 2, 8, 3, 3)
    R, s, step = torch.eye(3).expand(2, 8, 3, 3).contiguous(), torch.zeros(2, 8), torch.ones(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.smooth_step(h, R, s, step, 0.02, 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.smooth_backtrace(h, step)
    with pytest.raises(RuntimeError, match="SmoothHistory"):
        ops.smooth_step((h.R, None, h.delta, h.back), R, s, step, 0.02, 3.0)
    with pytest.raises(RuntimeError, match="SmoothHistory"):
        ops.smooth_backtrace(None, step)
    for bad in (-1.0, float("nan"), -INF):
        with pytest.raises(RuntimeError, match="jump"):
            ops._jump(bad)
    assert ops._jump(INF) == INF and ops._jump(0) == 0.0


def test_tracker_constructor_checks(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    T = ahv.track.PoseTracker
    for bad in (1, -1, -5):
        with pytest.raises(RuntimeError, match="history"):
            T(W1, W2, b2, particles=8, history=bad)
    with pytest.raises(RuntimeError, match="smooth_step"):
        T(W1, W2, b2, particles=8, history=4, backend=tr.make_backend(ahv, oracle))      # a backend without the smoother
    T(W1, W2, b2, particles=8, history=0, backend=tr.make_backend(ahv, oracle))          # ... is fine without history
    for kw, word in ((dict(smooth_sigma_deg=0.0), "smooth_sigma_deg"), (dict(smooth_sigma_deg=-1.0), "smooth_sigma_deg"),
                     (dict(smooth_sigma_deg=float("nan")), "smooth_sigma_deg"), (dict(smooth_jump=-1.0), "jump"),
                     (dict(smooth_jump=float("nan")), "jump"), (dict(sigma_deg=0.0), "smooth_sigma_deg")):
        with pytest.raises(RuntimeError, match=word):
            T(W1, W2, b2, particles=8, history=4, backend=sm.make_backend(ahv, oracle), **kw)
    t = T(W1, W2, b2, particles=8, sigma_deg=3.0, history=4, backend=sm.make_backend(ahv, oracle))
    assert t.smooth_sigma_deg == 3.0 and t.smooth_jump == 8.0 and t._hist.P is None
    t = T(W1, W2, b2, particles=8, sigma_deg=3.0, sigma_vel_deg=4.0, motion="constant_velocity", history=4,
          backend=sm.make_backend(ahv, oracle, cv.make_backend(ahv, oracle)))
    assert abs(t.smooth_sigma_deg - 5.0) < 1e-12 and t._hist.P is not None
    assert T(W1, W2, b2, particles=8, history=4, smooth_sigma_deg=1.5, smooth_jump=INF,
             backend=sm.make_backend(ahv, oracle)).smooth_sigma_deg == 1.5
    with pytest.raises(RuntimeError, match="history"):
        T(W1, W2, b2, particles=8).smoothed()
    with pytest.raises(RuntimeError, match="before the first step"):
        t.smoothed()


# ---- 3. the reference against brute force ------------------------------------------------------------------------------
def _tiny(ahv, M, T, seed, sigma_deg, dead=False):
    rs = np.random.RandomState(seed)
    base = ahv.rotations.haar_rotations_np(1, seed=seed)[0].astype(np.float64)
    Rs = [base @ tr.exp_so3(math.radians(2.0 * sigma_deg) * rs.standard_normal((M, 3))) for _ in range(T)]
    scores = [rs.uniform(-1, 1, M) for _ in range(T)]
    if dead:
        scores[T // 2][0] = np.nan
        scores[T - 1][M - 1] = -np.inf
    return Rs, scores


@pytest.mark.parametrize("M,T", [(1, 1), (1, 3), (2, 5), (3, 4), (4, 5), (4, 2)])
@pytest.mark.parametrize("jump", [0.0, 2.0, 8.0, INF])
def test_reference_equals_brute_force(ahv, M, T, jump):
    for seed, sigma_deg, dead in ((1, 3.0, False), (2, 30.0, False), (3, 10.0, True)):
        if dead and M == 1:
            continue
        Rs, scores = _tiny(ahv, M, T, seed, sigma_deg, dead)
        beta, sigma = 1.0 / 0.2, math.radians(sigma_deg)
        k = sm.inv4s2(sigma)
        ring = sm.Ring(T + 1, 1, M)
        for f in range(T):
            ring.step(f + 1, Rs[f][None], scores[f][None], beta, sigma, jump)
        idx, Rp = ring.backtrace(T, T)
        value, paths = sm.brute_force(Rs, Rs, scores, beta, k, jump)
        got = tuple(int(j) for j in idx[0])
        assert got in paths, (got, paths)
        assert abs(sm.path_value(got, Rs, Rs, scores, beta, k, jump) - value) <= 1e-12 * max(1.0, abs(value))
        # the recursion's own value of the best path: delta is kept relative to the running maximum m, the path value is not
        final = ring.delta[T % (T + 1), 0]
        assert int(np.argmax(np.where(np.isfinite(final), final, -np.inf))) == got[-1]
        for f, j in enumerate(got):
            assert np.array_equal(Rp[0, f], Rs[f][j])


def test_reference_with_velocities_equals_brute_force(ahv):
    M, T, jump, damping = 3, 4, 8.0, 0.8
    Rs, scores = _tiny(ahv, M, T, 5, 5.0)
    rs = np.random.RandomState(9)
    Vs = [math.radians(6.0) * rs.standard_normal((M, 3)) for _ in range(T)]
    Ps = [sm.predicted(R, V, damping) for R, V in zip(Rs, Vs)]
    sigma = math.radians(5.0)
    ring = sm.Ring(T, 1, M, velocities=True)                   # H = T: every slot in use
    for f in range(T):
        ring.step(f + 1, Rs[f][None], scores[f][None], 5.0, sigma, jump, V=Vs[f][None], damping=damping)
    got = tuple(int(j) for j in ring.backtrace(T, T)[0][0])
    value, paths = sm.brute_force(Rs, Ps, scores, 5.0, sm.inv4s2(sigma), jump)
    assert got in paths and abs(sm.path_value(got, Rs, Ps, scores, 5.0, sm.inv4s2(sigma), jump) - value) < 1e-12


def test_jump_zero_is_the_per_frame_argmax(ahv):
    M, T = 4, 5
    for seed in (1, 2, 3):
        Rs, scores = _tiny(ahv, M, T, seed, 3.0)
        ring = sm.Ring(3, 1, M)                                 # the ring wraps
        paths = []
        for f in range(T):
            ring.step(f + 1, Rs[f][None], scores[f][None], 50.0, math.radians(3.0), 0.0)
            paths.append(ring.backtrace(f + 1, min(f + 1, 3))[0][0])
        assert [int(p[-1]) for p in paths] == [int(np.argmax(s)) for s in scores]
        assert list(paths[-1]) == [int(np.argmax(s)) for s in scores[-3:]]
        # every transition costs exactly 0 = -jump, so delta - a is 0 and back is the first arg-max of the frame before
        assert np.array_equal(ring.back[T % 3, 0], np.full(M, int(np.argmax(scores[-2])), np.int32))


def test_backtrace_break_rule(ahv):
    M, H = 3, 8
    Rs, scores = _tiny(ahv, M, 7, 4, 3.0)
    scores[3][:] = np.nan                                       # frame 4: every score non-finite
    scores[5][1] = np.inf                                       # frame 6: one dead particle
    ring = sm.Ring(H, 2, M)
    both = lambda x: np.stack([x, x[::-1]])
    for f in range(7):
        ring.step(f + 1, both(Rs[f]), both(scores[f]), 5.0, math.radians(3.0), 8.0)
    assert np.all(ring.delta[4 % H] == -np.inf) and np.all(ring.back[4 % H] == -1)
    assert np.all(ring.back[5 % H] == -1)                        # frame 5 has no live predecessor: it restarts
    assert np.array_equal(ring.delta[5 % H, 0], 5.0 * scores[4])
    assert ring.delta[6 % H, 0, 1] == -np.inf and ring.back[6 % H, 0, 1] == -1
    idx, Rp = ring.backtrace(7, 8)                               # more frames than were recorded
    for b in range(2):
        assert idx[b, 0] == -1 and np.array_equal(Rp[b, 0], np.eye(3))          # frame 0: before first_step
        assert idx[b, 4] == -1 and np.array_equal(Rp[b, 4], np.eye(3))          # frame 4: the dead frame
        assert idx[b, 3] == int(np.argmax(ring.delta[3 % H, b]))                 # behind the break: that frame's own arg-max
        assert idx[b, 7] == int(np.argmax(np.where(np.isfinite(ring.delta[7 % H, b]), ring.delta[7 % H, b], -np.inf)))
        assert all(idx[b, f] >= 0 for f in (1, 2, 3, 5, 6, 7))
        for f in (2, 3, 6, 7):                                                    # the chain follows back[]
            assert idx[b, f - 1] == ring.back[f % H, b, idx[b, f]]
    # a later first_step hides the older frames
    idx2, _ = ring.backtrace(7, 8, first_step=6)
    assert np.all(idx2[:, :6] == -1) and np.array_equal(idx2[:, 6:], idx[:, 6:])


# ---- 4. the control flow on the oracle backend -------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_tracker_control_flow(ahv, oracle, g128, motion):
    W1, W2, b2 = _head(g128)
    B, M, N0, H = 2, 24, 40, 4
    vs, vt = _pair(B)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    calls = WALK_CALLS if motion == "walk" else CV_CALLS
    mk = lambda: cv.make_backend(ahv, oracle)
    kw = dict(particles=M, sigma_deg=4.0, n_fresh=5, temperature=0.05, batch=B, seed=3, motion=motion, sigma_vel_deg=1.5, damping=0.9)

    def run(history):
        be = sm.make_backend(ahv, oracle, mk())
        t = ahv.track.PoseTracker(W1, W2, b2, backend=be, history=history, **kw)
        t.init(vs, vt, R0)
        assert "smooth_step" not in be.calls            # init records nothing
        outs, paths = [], []
        for n in range(1, 7):
            be.calls.clear()
            o = t.step(vs, vt)
            assert be.calls == calls + (["smooth_step"] if history else []), be.calls
            outs.append([x.clone() if isinstance(x, torch.Tensor) else x for x in o])
            if history:
                ls = be.last_smooth
                assert ls["t"] == n and ls["first_step"] == 1 and ls["jump"] == 8.0
                assert abs(ls["sigma_deg"] - (4.0 if motion == "walk" else math.hypot(4.0, 1.5))) < 1e-12
                assert (ls["V"] is None) if motion == "walk" else (ls["V"].data_ptr() == t.velocities.data_ptr() and ls["damping"] == 0.9)
                p = t.smoothed()
                assert tuple(p.idx.shape) == (B, min(n, H)) and tuple(p.R.shape) == (B, min(n, H), 3, 3)
                assert tuple(t.smoothed(frames=2).idx.shape) == (B, min(n, 2))
                assert torch.equal(t.smoothed(frames=2).idx, p.idx[:, -2:][:, -min(n, 2):])
                # the newest frame of the path is a particle of this step
                rows = torch.arange(B)
                assert torch.equal(p.R[:, -1], o.particles[rows, p.idx[:, -1]])
                paths.append(p)
        return t, be, outs, paths

    t0, _, plain, _ = run(0)
    t1, be, smooth, paths = run(H)
    for a, b in zip(plain, smooth):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)         # smoothing observes, never steers
    # the ring holds what the reference computes from the recorded sets
    slot = 6 % H
    assert torch.equal(t1._hist.R[slot], smooth[-1][3])
    # a new init hides the old slots: after one more step the path has one frame
    t1.init(vs, vt, R0)
    with pytest.raises(RuntimeError, match="before the first step"):
        t1.smoothed()
    t1.step(vs, vt)
    assert tuple(t1.smoothed().idx.shape) == (B, 1)
    assert int(be.last_smooth["t"]) == 1
    assert (t1._hist.back[1 % H] == -1).all()                                # no predecessors behind first_step


def test_track_sequence_smoothed_keyword(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    item = next(iter(ahv.harness.SyntheticSequences(n_seq=1, n_frames=6, seed=3)))
    vols = {}

    class Model:
        def forward_features(self, a, b):
            f = lambda x: vols.setdefault(float(x.flatten()[0]), torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return f(a), f(b)

    props = torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9))
    mk = lambda **kw: ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=sm.make_backend(ahv, oracle), **kw)
    plain = ahv.harness.track_sequence(Model(), item, mk(), ref=0, proposals=props, device="cpu")
    assert sorted(plain) == ["R_map", "err", "frames", "score"]                    # the default result is unchanged
    res = ahv.harness.track_sequence(Model(), item, mk(history=3), ref=0, proposals=props, device="cpu", smoothed=True)
    for k in plain:
        assert (plain[k] == res[k]) if k == "frames" else torch.equal(plain[k], res[k])
    s = res["smoothed"]
    assert s["frames"] == [3, 4, 5] and tuple(s["R"].shape) == (3, 3, 3) and tuple(s["idx"].shape) == (3,) and tuple(s["err"].shape) == (3,)
    for k, f in enumerate(s["frames"]):
        R_gt = item["R"][f] @ item["R"][0].T
        assert abs(float(s["err"][k]) - float(ahv.rotations.geodesic_deg(s["R"][k][None], R_gt[None]))) < 1e-4
    with pytest.raises(RuntimeError, match="history"):
        ahv.harness.track_sequence(Model(), item, mk(), ref=0, proposals=props, device="cpu", smoothed=True)


# ---- 5. the planted sequence with two distractor frames ----------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_distractor(ahv, oracle, g128, s):
    """track_reference.PLANTED with frames 5 and 8 replaced by an unrelated view; history 12, smoothing sigma 3 degrees, jump 8.
    Measured on the oracle backend with numpy noise, degrees.  The filter's reported pose on frames 5 / 8: 161.5 / 135.0,
    159.2 / 158.7 and 169.0 / 127.3 off for s = 0, 1, 2.  The smoothed path's largest error over frames 4-11 against the blind
    4 096-hypothesis median of the clean sequence: 3.74 / 8.44, 2.24 / 8.00 and 1.46 / 7.01."""
    P = sm.DISTRACTED
    W1, W2, b2 = _head(g128)
    vs = torch.from_numpy(np.ascontiguousarray(g128["vol_src"]))
    R0 = torch.from_numpy(tr.planted_init(ahv.rotations, s))
    w = [x.numpy() for x in (W1, W2, b2)]
    t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                              temperature=P["temperature"], batch=1, seed=s, backend=sm.make_backend(ahv, oracle),
                              history=P["history"], smooth_sigma_deg=P["smooth_sigma_deg"], smooth_jump=P["smooth_jump"])
    rotate = lambda R: torch.from_numpy(oracle.rotate_volume(vs.numpy(), R[None].astype(np.float32)))
    filt, smooth = sm.distracted_run(ahv.rotations, s, rotate, lambda vt: t.init(vs, vt, R0), lambda vt: t.step(vs, vt), t.smoothed)
    gt = tr.planted_truth(ahv.rotations, s)
    blind = []
    for k in range(P["frames"]):
        vt = rotate(gt[k])
        Rb = R0.numpy()[int(oracle.score_hypotheses(vs.numpy(), vt.numpy(), R0.numpy(), *w)[2][0])]
        blind.append(float(tr.geodesic_deg(Rb.astype(np.float64), gt[k])))
    worst, median = sm.distracted_bar(smooth, blind)
    print("distractor s=%d: filter %s | smoothed (frames 1-11) %s | smoothed max over 4-11 %.3f | blind median %.3f"
          % (s, " ".join("%.2f" % e for e in filt), " ".join("%.2f" % e for e in smooth), worst, median))
    for k in P["distractors"]:
        assert filt[k] > 90.0, (k, filt[k])               # the premise: the filter follows the distractor
    assert worst < median
