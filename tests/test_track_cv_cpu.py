"""Constant-velocity pose tracking, CPU tier: argument validation of ``ahv_predict_rotations_f32`` through the ctypes table
(validation runs before any HIP call), the host-side checks of ``ops.predict_rotations``, the control flow of
``track.PoseTracker(motion="constant_velocity")`` on an oracle-backed backend (tests/track_cv_reference.py), and the planted
sequences: the fast one (9 degrees per frame), where the random walk is lost, and track_reference.PLANTED (3 degrees per frame)."""
import os
import re

import numpy as np
import pytest
import torch

from . import resample_reference as rr
from . import track_cv_reference as cv
from . import track_reference as tr
from .conftest import REPO

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


# ---- 1. the entry point refuses bad arguments before any HIP call ----------------------------------------------------
def test_predict_argument_validation_needs_no_gpu(lib):
    f = lib.ahv_predict_rotations_f32
    # (0 idx, 1 R, 2 r_batch_stride, 3 V, 4 v_batch_stride, 5 N, 6 best_key, 7 M, 8 n_fresh, 9 B, 10 seed, 11 step, 12 sigma,
    #  13 sigma_vel, 14 damping, 15 max_angle, 16 max_speed, 17 coast, 18 out, 19 vel_out, 20 omega, 21 stream)
    ok = [None, 1, 0, None, 0, 10, None, 8, 0, 2, 0, 1, 0.05, 0.02, 1.0, 0.0, 0.0, 1, 1, 1, None, None]

    def refused(word, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert f(*a) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(b"predict_rotations") and word in msg, (kw, msg)

    refused(b"null", _1=None)                    # R
    refused(b"null", _18=None)                   # out
    refused(b"null", _19=None)                   # vel_out
    refused(b"null", _11=None)                   # step
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _7=bad)
    for bad in (0, -1):
        refused(b"empty rotation set", _5=bad)
    for bad in (-1, 9):
        refused(b"n_fresh", _8=bad)
    for bad in (0, 65536):
        refused(b"B =", _9=bad)
    for bad in (9, 89):
        refused(b"r_batch_stride", _2=bad)
    for bad in (3, 29, 90):
        refused(b"v_batch_stride", _4=bad)
        refused(b"v_batch_stride", _3=1, _4=bad)
    for slot, word in ((12, b"sigma ="), (13, b"sigma_vel"), (15, b"max_angle"), (16, b"max_speed")):
        for bad in (-0.1, float("inf"), float("nan")):
            refused(word, **{"_%d" % slot: bad})
    for bad in (-0.01, 1.01, float("inf"), float("nan")):
        refused(b"damping", _14=bad)


def test_abi_version_unchanged_and_prototype_agrees(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bahv_predict_rotations_f32\s*\(([^;]*)\)\s*;", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(ahv._lib.SIGNATURES["ahv_predict_rotations_f32"][1]) == 22


# ---- 2. the op checks on the host ------------------------------------------------------------------------------------
def test_op_checks_arguments_before_any_launch(ahv):
    ops = ahv.ops
    R = torch.eye(3)[None].repeat(4, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.predict_rotations(R, step=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.predict_rotations(R, V=torch.zeros(4, 3), step=torch.zeros(1, dtype=torch.int64))
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="damping"):
            ops._unit_interval(bad, "damping")
    assert ops._unit_interval(0, "damping") == 0.0 and ops._unit_interval(1, "damping") == 1.0


def test_tracker_constructor_checks(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    T = ahv.track.PoseTracker
    for kw, word in ((dict(motion="velocity"), "motion"), (dict(motion=None), "motion"),
                     (dict(motion="constant_velocity", sigma_vel_deg=-1), "sigma_vel_deg"),
                     (dict(motion="constant_velocity", sigma_vel_deg=float("nan")), "sigma_vel_deg"),
                     (dict(motion="constant_velocity", damping=1.5), "damping"),
                     (dict(motion="constant_velocity", damping=float("nan")), "damping"),
                     (dict(motion="constant_velocity", max_speed_deg=-2.0), "max_speed_deg"),
                     (dict(motion="constant_velocity", max_speed_deg=float("inf")), "max_speed_deg")):
        with pytest.raises(RuntimeError, match=word):
            T(W1, W2, b2, particles=8, **kw)
    with pytest.raises(RuntimeError, match="use_graph"):
        T(W1, W2, b2, particles=8, motion="constant_velocity", use_graph=True, backend=cv.make_backend(ahv, oracle))
    t = T(W1, W2, b2, particles=8, motion="constant_velocity")
    assert t.velocities is None
    with pytest.raises(RuntimeError, match="init"):
        t.step(torch.zeros(1, 16, 8, 8, 8), torch.zeros(1, 16, 8, 8, 8))
    assert T(W1, W2, b2, particles=8).velocities is None and T(W1, W2, b2, particles=8).motion == "walk"


# ---- 3. the control flow on the oracle backend -------------------------------------------------------------------------
@pytest.mark.parametrize("coast", [True, False])
def test_tracker_control_flow(ahv, oracle, g128, coast):
    W1, W2, b2 = _head(g128)
    B, M, N0, F, damping, T = 2, 24, 40, 5, 0.9, 0.05
    vs, vt = _pair(B)
    be = cv.make_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=4.0, n_fresh=F, temperature=T, batch=B, seed=3, backend=be,
                              motion="constant_velocity", sigma_vel_deg=1.5, damping=damping, coast=coast)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    prev = t.init(vs, vt, R0)
    assert t.velocities is None and not prev.reacquired.any() and int(t.step_counter[0]) == 0
    V_prev, ptrs = None, {}
    rows = np.arange(B)
    for n in range(1, 7):
        be.calls.clear()
        out = t.step(vs, vt)
        V = t.velocities
        assert be.calls == CV_CALLS
        assert int(t.step_counter[0]) == n
        assert tuple(out.particles.shape) == (B, M, 3, 3) and tuple(V.shape) == (B, M, 3) and V.dtype == torch.float32
        # the backend was handed the velocities of the previous step (none on the first step after init)
        assert (be.last_V is None) if n == 1 else np.array_equal(be.last_V, V_prev)
        # the step is the reference's, given the backend's random numbers
        draws = rr.resample(prev.scores.numpy(), M, T, be.last_u)
        best = prev.scores.numpy().argmax(axis=1)
        want, want_v, _ = cv.predict(prev.particles.numpy(), V_prev, draws, be.last_omega, be.last_accel, damping, best_idx=best,
                                     coast=coast, fresh=be.last_fresh)
        assert np.array_equal(out.draws.numpy(), draws)
        assert np.array_equal(out.particles.numpy(), want.astype(np.float32))
        assert np.array_equal(V.numpy(), want_v.astype(np.float32))
        # slot 0: the previous arg-max and its velocity, bit for bit
        v_best = np.zeros((B, 3), np.float32) if V_prev is None else V_prev[rows, best]
        assert torch.equal(out.particles[:, 0], prev.R_map)
        assert np.array_equal(V[:, 0].numpy(), v_best)
        lo = 2 if coast else 1
        if coast:   # slot 1: the previous arg-max moved by its own velocity, which it keeps
            assert np.array_equal(V[:, 1].numpy(), v_best)
            moved = prev.R_map.double().numpy() @ tr.exp_so3(v_best.astype(np.float64))
            assert np.array_equal(out.particles[:, 1].numpy(), moved.astype(np.float32))
            if n == 1:
                assert torch.equal(out.particles[:, 1], prev.R_map)
        # the other slots' velocities are the previous ones gathered through the draws, damped, plus the backend's noise
        vg = np.zeros((B, M, 3)) if V_prev is None else cv.gather_vel(V_prev.astype(np.float64), draws)
        assert np.array_equal(V[:, lo:M - F].numpy(), (damping * vg + be.last_accel)[:, lo:M - F].astype(np.float32))
        assert not V[:, M - F:].any() and np.array_equal(out.particles[:, M - F:].numpy(), be.last_fresh)
        if n > 1:
            assert np.abs(vg[:, lo:M - F]).max() > 0
        # scores, winner, reacquired
        s, _, _ = oracle.score_hypotheses(vs.numpy(), vt.numpy(), out.particles.numpy(), W1.numpy(), W2.numpy(), b2.numpy())
        assert np.array_equal(out.scores.numpy(), s)
        assert torch.equal(out.idx, out.scores.argmax(dim=1))
        assert torch.equal(out.R_map, out.particles[torch.arange(B), out.idx])
        assert torch.equal(out.reacquired, out.idx >= max(M - F, lo))
        assert (out.score >= prev.score).all()          # same frame, elite kept: the score never decreases
        # ping-pong: a step writes the half the previous one did not; from step 3 on every pointer has been seen before
        now = tuple(x.data_ptr() for x in (out.score, out.idx, out.R_map, out.particles, out.scores, out.draws, out.reacquired, V))
        assert out.particles.data_ptr() != prev.particles.data_ptr()
        if n >= 3:
            assert now == ptrs[n - 2], "a step allocated an output"
        if n >= 2:
            assert now[3] != ptrs[n - 1][3] and now[7] != ptrs[n - 1][7] and now[5] == ptrs[n - 1][5]
        ptrs[n] = now
        prev, V_prev = out, V.numpy().copy()
    t.init(vs, vt, R0)
    assert t.velocities is None            # a new init starts from zero velocities again


def test_reacquired_when_every_slot_is_fresh(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(1)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(16, seed=5))
    for coast, lo in ((True, 2), (False, 1)):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=6, n_fresh=6, batch=1, seed=1, backend=cv.make_backend(ahv, oracle),
                                  motion="constant_velocity", coast=coast)
        t.init(vs, vt, R0)
        for _ in range(3):
            out = t.step(vs, vt)
            assert torch.equal(out.reacquired, out.idx >= lo)


def test_walk_issues_todays_calls_and_bytes(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(2)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(40, seed=5))

    def run(backend, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=24, sigma_deg=4.0, n_fresh=5, temperature=0.05, batch=2, seed=3,
                                  backend=backend, **kw)
        t.init(vs, vt, R0)
        outs = []
        for _ in range(3):
            backend.calls.clear()
            outs.append(t.step(vs, vt).particles.clone())
            assert backend.calls == WALK_CALLS
            assert t.velocities is None
        return outs

    a = run(tr.make_backend(ahv, oracle))                              # a backend without predict_rotations
    b = run(cv.make_backend(ahv, oracle), motion="walk", sigma_vel_deg=2.0, damping=0.5, coast=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_track_sequence_accepts_a_constant_velocity_tracker(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    item = next(iter(ahv.harness.SyntheticSequences(n_seq=1, n_frames=5, seed=3)))
    vols = {}

    class Model:
        def forward_features(self, a, b):
            f = lambda x: vols.setdefault(float(x.flatten()[0]), torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return f(a), f(b)

    be = cv.make_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=be, motion="constant_velocity")
    res = ahv.harness.track_sequence(Model(), item, t, ref=0, proposals=torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9)),
                                     device="cpu")
    assert res["frames"] == [1, 2, 3, 4] and tuple(res["R_map"].shape) == (4, 3, 3)
    assert int(t.step_counter[0]) == 3 and be.calls.count("predict_rotations") == 3 and "diffuse_rotations" not in be.calls
    assert tuple(t.velocities.shape) == (1, 16, 3) and torch.isfinite(res["score"]).all()


# ---- 4. the planted sequences ------------------------------------------------------------------------------------------
def _planted(ahv, oracle, g128, s, P, motions):
    """name -> (init_frame, step_frame) of one tracker per motion on planted sequence s, and ``rotate``."""
    W1, W2, b2 = _head(g128)
    vs = torch.from_numpy(np.ascontiguousarray(g128["vol_src"]))
    R0 = torch.from_numpy(tr.planted_init(ahv.rotations, s))
    trackers = {}
    for motion in motions:
        t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                  temperature=P["temperature"], batch=1, seed=s, backend=cv.make_backend(ahv, oracle), motion=motion,
                                  sigma_vel_deg=cv.FAST["sigma_vel_deg"], damping=cv.FAST["damping"])
        trackers[motion] = (lambda vt, t=t: t.init(vs, vt, R0), lambda vt, t=t: t.step(vs, vt))
    rotate = lambda R: torch.from_numpy(oracle.rotate_volume(vs.numpy(), R[None].astype(np.float32)))
    return trackers, rotate, vs, R0


@pytest.mark.parametrize("s", [0, 1, 2])
def test_fast_planted_sequence(ahv, oracle, g128, s):
    """9 degrees per frame, 256 particles, sigma 3, sigma_vel 1, damping 1, 16 fresh slots, T = 0.02; both trackers on the same
    frames with the same seed.  Measured on the oracle backend with numpy noise (constant-velocity late max / walk late median
    over frames 8-15, degrees): 1.70 / 18.49, 1.48 / 21.30 and 1.48 / 13.53 for s = 0, 1, 2."""
    trackers, rotate, _, _ = _planted(ahv, oracle, g128, s, cv.FAST, ("walk", "constant_velocity"))
    err = cv.run(ahv.rotations, s, cv.FAST, rotate, trackers)
    worst, median = cv.fast_bar(err["constant_velocity"], err["walk"])
    for name in ("walk", "constant_velocity"):
        print("fast planted s=%d %-17s: %s" % (s, name, " ".join("%.2f" % e for e in err[name])))
    print("fast planted s=%d: constant-velocity late max %.3f | walk late median %.3f" % (s, worst, median))
    assert worst < median


@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_moving_optimum_with_constant_velocity(ahv, oracle, g128, s):
    """track_reference.PLANTED itself (3 degrees per frame, 512 particles): the constant-velocity tracker meets the bar of the
    walk tracker, late max below the blind median.  Measured on the oracle backend with numpy noise (late max / blind median,
    degrees): 1.24 / 8.44, 0.96 / 8.00 and 1.10 / 7.01 for s = 0, 1, 2."""
    P = tr.PLANTED
    trackers, rotate, vs, R0 = _planted(ahv, oracle, g128, s, P, ("constant_velocity",))
    w = [x.numpy() for x in _head(g128)]

    class T:
        init_frame, step_frame = (staticmethod(f) for f in trackers["constant_velocity"])

    blind = lambda vt: R0.numpy()[int(oracle.score_hypotheses(vs.numpy(), vt.numpy(), R0.numpy(), *w)[2][0])]
    track, blind_err = tr.planted_run(ahv.rotations, s, rotate, T, blind)
    worst, median = tr.planted_bar(track, blind_err)
    print("planted s=%d, constant velocity: tracker %s | late max %.3f | blind median %.3f"
          % (s, " ".join("%.2f" % e for e in track), worst, median))
    assert worst < median
