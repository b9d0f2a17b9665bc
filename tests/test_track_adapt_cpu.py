"""Noise scale and fresh slots adapted on the device, CPU tier: argument validation of ``ahv_track_control_f32`` and
``ahv_predict_rotations_ctl_f32`` through the ctypes table (validation runs before any HIP call), the host-side checks of the
ops, the constructor, the control flow of ``track.PoseTracker(adapt=...)`` on an oracle-backed backend
(tests/track_adapt_reference.py), the conditions of the control kernel's cases, and the three planted sequences."""
import math
import os
import re

import numpy as np
import pytest
import torch

from . import track_adapt_reference as ar
from . import track_cv_reference as cv
from . import track_reference as tr
from .conftest import REPO

WALK_CALLS = ["track_advance", "resample", "diffuse_rotations", "verify_pair", "select_rotation"]
CV_CALLS = ["track_advance", "resample", "predict_rotations", "verify_pair", "select_rotation"]
ADAPT_CALLS = ["track_advance", "resample", "predict_rotations_controlled", "verify_pair", "select_rotation", "track_control"]
FIELDS = ("score", "idx", "R_map", "particles", "scores", "draws", "reacquired")


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


# ---- 1. the entry points refuse bad arguments before any HIP call ----------------------------------------------------
def _refuser(lib, f, ok, prefix):
    def refused(word, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert f(*a) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(prefix) and word in msg, (kw, msg)
    return refused


def test_control_argument_validation_needs_no_gpu(lib):
    # (0 R_cur, 1 V_cur, 2 idx, 3 score, 4 B, 5 M, 6 first, 7 sigma0, 8 sigma_vel0, 9 n_fresh0, 10 sigma_min, 11 sigma_max, 12 gain,
    #  13 rate, 14 score_floor, 15 n_fresh_lost, 16 control, 17 reacquired, 18 stream)
    ok = [1, None, 1, 1, 2, 8, 1, 0.05, 0.02, 2, 0.01, 0.1, 1.5, 0.5, -math.inf, 8, 1, 1, None]
    refused = _refuser(lib, lib.ahv_track_control_f32, ok, b"track_control")
    for slot in (0, 2, 3, 16, 17):
        refused(b"null", **{"_%d" % slot: None})
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _5=bad)
    for bad in (0, 65536):
        refused(b"B =", _4=bad)
    for bad in (0, 3, -1):
        refused(b"first", _6=bad)
    nan, inf = float("nan"), float("inf")
    for bad in (0.0, -0.1, inf, nan):
        refused(b"sigma_min", _10=bad)
        refused(b"sigma_min", _11=bad)
        refused(b"sigma0", _7=bad)
        refused(b"gain", _12=bad)
    refused(b"sigma_min", _10=0.2, _11=0.1)           # min above max
    for bad in (-0.1, inf, nan):
        refused(b"sigma_vel0", _8=bad)
    for bad in (0.0, -0.5, 1.01, inf, nan):
        refused(b"rate", _13=bad)
    refused(b"score_floor", _14=nan)
    for bad in (-1, 9):
        refused(b"n_fresh0", _9=bad)
        refused(b"n_fresh_lost", _15=bad)


def test_predict_ctl_argument_validation_needs_no_gpu(lib):
    # (0 idx, 1 R, 2 r_batch_stride, 3 V, 4 v_batch_stride, 5 N, 6 best_key, 7 M, 8 control, 9 B, 10 seed, 11 step, 12 damping,
    #  13 max_angle, 14 max_speed, 15 coast, 16 out, 17 vel_out, 18 omega, 19 stream)
    ok = [None, 1, 0, None, 0, 10, None, 8, 1, 2, 0, 1, 1.0, 0.0, 0.0, 1, 1, 1, None, None]
    refused = _refuser(lib, lib.ahv_predict_rotations_ctl_f32, ok, b"predict_rotations_ctl")
    for slot in (1, 8, 11, 16):
        refused(b"null", **{"_%d" % slot: None})
    refused(b"vel_out is required", _17=None)                 # coast slot without vel_out
    refused(b"vel_out is required", _17=None, _15=0, _3=1)    # V without vel_out
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _7=bad)
    for bad in (0, -1):
        refused(b"empty rotation set", _5=bad)
    for bad in (0, 65536):
        refused(b"B =", _9=bad)
    for bad in (9, 89):
        refused(b"r_batch_stride", _2=bad)
    for bad in (3, 29, 90):
        refused(b"v_batch_stride", _4=bad)
    for slot, word in ((13, b"max_angle"), (14, b"max_speed")):
        for bad in (-0.1, float("inf"), float("nan")):
            refused(word, **{"_%d" % slot: bad})
    for bad in (-0.01, 1.01, float("inf"), float("nan")):
        refused(b"damping", _12=bad)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    assert int(re.search(r"#define\s+AHV_TRACK_CONTROL_WORDS\s+(\d+)", text).group(1)) == ahv._lib.AHV_TRACK_CONTROL_WORDS == ar.WORDS == 8
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("ahv_track_control_f32", 19), ("ahv_predict_rotations_ctl_f32", 20)):
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(ahv._lib.SIGNATURES[name][1]) == count


# ---- 2. the ops check on the host --------------------------------------------------------------------------------------
def test_record_helpers_and_host_checks(ahv):
    ops = ahv.ops
    rec = ops.track_control_state(3, 3.0, 1.0, 16, "cpu")
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (3, 8)
    assert np.array_equal(rec.numpy(), ar.fresh_record(3, 3.0, 1.0, 16))
    d = ops.decode_track_control(rec)
    assert d._fields == ("sigma_deg", "sigma_vel_deg", "n_fresh", "lost", "reacquired", "updated", "innovation_deg", "score")
    assert all(tuple(x.shape) == (3,) for x in d)
    assert torch.allclose(d.sigma_deg, torch.full((3,), 3.0)) and torch.allclose(d.sigma_vel_deg, torch.full((3,), 1.0))
    assert d.n_fresh.tolist() == [16] * 3 and not (d.lost.any() or d.reacquired.any() or d.updated.any())
    assert torch.isnan(d.innovation_deg).all() and torch.isnan(d.score).all()
    flags = ar.pack(0.1, 0.05, 7, np.array([1, 2, 4, 7]), 0.01, 0.02, 0.9)
    d = ops.decode_track_control(torch.from_numpy(flags))
    assert d.lost.tolist() == [True, False, False, True] and d.reacquired.tolist() == [False, True, False, True]
    assert d.updated.tolist() == [False, False, True, True] and d.n_fresh.tolist() == [7] * 4
    for bad in (torch.zeros(3, 8), torch.zeros(3, 7, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match="control must be"):
            ops.decode_track_control(bad)
    for kw, word in ((dict(B=0), "B ="), (dict(sigma_deg=-1.0), "sigma_deg"), (dict(sigma_vel_deg=float("nan")), "sigma_vel_deg"),
                     (dict(n_fresh=-1), "n_fresh")):
        with pytest.raises(RuntimeError, match=word):
            ops.track_control_state(**dict(dict(B=2, sigma_deg=3.0, sigma_vel_deg=1.0, n_fresh=0, device="cpu"), **kw))
    # no CPU path
    R, step = torch.eye(3).repeat(2, 4, 1, 1), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.predict_rotations_controlled(R, rec[:2], step=step, velocities=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_control(rec[:2], R, torch.zeros(2, dtype=torch.int64), torch.zeros(2))


def test_tracker_constructor_checks(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    T, A = ahv.track.PoseTracker, ahv.track.AdaptiveNoise
    a = A()
    assert (a.sigma_min_deg, a.sigma_max_deg, a.gain, a.rate, a.score_floor, a.n_fresh_lost) == (0.5, 8.0, 1.5, 0.5, None, None)
    for kw, word in ((dict(sigma_min_deg=0.0), "sigma_min"), (dict(sigma_min_deg=9.0), "sigma_min"), (dict(sigma_max_deg=float("inf")), "sigma_max"),
                     (dict(gain=0.0), "gain"), (dict(gain=float("nan")), "gain"), (dict(rate=0.0), "rate"), (dict(rate=1.5), "rate"),
                     (dict(score_floor=float("nan")), "score_floor"), (dict(n_fresh_lost=-1), "n_fresh_lost")):
        with pytest.raises(RuntimeError, match=word):
            A(**kw)
    assert A(score_floor=float("-inf")).score_floor == -math.inf
    be = ar.make_backend(ahv, oracle)
    sym = object()      # refused before anything looks at it
    for kw, word in ((dict(adapt=a, backend=cv.make_backend(ahv, oracle)), "predict_rotations_controlled and track_control"),
                     (dict(adapt=a, backend=be, symmetry=sym), "not built"),
                     (dict(adapt=a, backend=be, views=torch.eye(3)[None]), "not built"),
                     (dict(adapt=a, backend=be, history=4), "smooth_sigma_deg"),
                     (dict(adapt=a, backend=be, sigma_deg=0.0), "sigma_deg > 0"),
                     (dict(adapt=A(n_fresh_lost=9), backend=be), "n_fresh_lost"),
                     (dict(adapt=dict(gain=1.5), backend=be), "AdaptiveNoise")):
        with pytest.raises(RuntimeError, match=word):
            T(W1, W2, b2, particles=8, **kw)
    t = T(W1, W2, b2, particles=8, n_fresh=2, adapt=a, backend=be, batch=2)
    assert np.array_equal(t.control_record.numpy(), ar.fresh_record(2, 3.0, 0.0, 2))       # the walk has no velocity noise
    assert t.control().n_fresh.tolist() == [2, 2]
    plain = T(W1, W2, b2, particles=8)
    assert plain.control_record is None and plain.adapt is None
    with pytest.raises(RuntimeError, match="adapt="):
        plain.control()


# ---- 3. the control flow on the oracle backend -------------------------------------------------------------------------
@pytest.mark.parametrize("motion,coast", [("walk", False), ("constant_velocity", True), ("constant_velocity", False)])
def test_adaptive_tracker_control_flow(ahv, oracle, g128, motion, coast):
    W1, W2, b2 = _head(g128)
    B, M, N0, F, T = 2, 24, 40, 5, 0.05
    cvm = motion != "walk"
    vs, vt = _pair(B)
    be = ar.make_backend(ahv, oracle)
    rule = ahv.track.AdaptiveNoise(sigma_min_deg=1.0, sigma_max_deg=20.0, gain=1.5, rate=0.5, score_floor=0.05, n_fresh_lost=12)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=4.0, n_fresh=F, temperature=T, batch=B, seed=3, backend=be,
                              motion=motion, sigma_vel_deg=1.5, damping=0.9, coast=coast, adapt=rule)
    first = 2 if cvm and coast else 1
    p = ar.params(first, 4.0, 1.5 if cvm else 0.0, F, 1.0, 20.0, 1.5, 0.5, 0.05, 12)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    prev = t.init(vs, vt, R0)
    rec = ar.fresh_record(B, 4.0, 1.5 if cvm else 0.0, F)
    assert np.array_equal(t.control_record.numpy(), rec)
    V_prev, seen = None, set()
    for n in range(1, 7):
        be.calls.clear()
        out = t.step(vs, vt)
        assert be.calls == ADAPT_CALLS
        assert int(t.step_counter[0]) == n
        assert np.array_equal(be.last_record, rec)          # the predict step read the record the last decision left
        old = ar.unpack(rec)
        nf = np.clip(old["n_fresh"], 0, M)
        # the particles: the reference's, given the backend's random numbers and the record's sigma and n_fresh
        draws = tr.rr.resample(prev.scores.numpy(), M, T, be.last_u)
        best = prev.scores.numpy().argmax(axis=1)
        assert np.array_equal(out.draws.numpy(), draws)
        Pp = prev.particles.numpy()
        for b in range(B):
            fresh = be.last_fresh[b:b + 1, :nf[b]] if nf[b] else None
            Pb = Pp[b:b + 1] if Pp.ndim == 4 else Pp          # (init scored one shared set)
            if cvm:
                want, want_v, _ = cv.predict(Pb, None if V_prev is None else V_prev[b:b + 1], draws[b:b + 1],
                                             be.last_omega[b:b + 1], be.last_accel[b:b + 1], 0.9, best_idx=best[b:b + 1], coast=coast,
                                             fresh=fresh)
                assert np.array_equal(t.velocities.numpy()[b:b + 1], want_v.astype(np.float32))
            else:
                want = tr.diffuse(Pb, draws[b:b + 1], be.last_omega[b:b + 1], best_idx=best[b:b + 1], fresh=fresh)
            got = out.particles.numpy()[b:b + 1]
            assert np.array_equal(got[:, 1:], want.astype(np.float32)[:, 1:])
        assert torch.equal(out.particles[:, 0], prev.R_map)          # slot 0: the previous MAP pose, bit for bit
        assert t.velocities is None if not cvm else tuple(t.velocities.shape) == (B, M, 3)
        # the decision: the reference rule on the step's own outputs
        Vn = t.velocities.numpy() if cvm else None
        rec, reacq = ar.control_record(rec, out.particles.numpy(), Vn, out.idx.numpy(), out.score.numpy(), p)
        assert np.array_equal(t.control_record.numpy().view(np.uint32), rec.view(np.uint32))
        assert np.array_equal(out.reacquired.numpy(), reacq)
        assert np.array_equal(reacq, out.idx.numpy() >= np.maximum(M - nf, first))
        d = t.control()
        assert d.lost.tolist() == (out.score.numpy() < np.float32(0.05)).tolist()
        seen.update(int(x) for x in ar.unpack(rec)["n_fresh"])
        prev, V_prev = out, (t.velocities.numpy().copy() if cvm else None)
    t.init(vs, vt, R0)
    assert np.array_equal(t.control_record.numpy(), ar.fresh_record(B, 4.0, 1.5 if cvm else 0.0, F))      # init resets the record
    assert seen <= {F, 12}


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_adapt_none_issues_todays_calls_and_bytes(ahv, oracle, g128, motion):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(2)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(40, seed=5))

    def run(backend, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=24, sigma_deg=4.0, n_fresh=5, temperature=0.05, batch=2, seed=3,
                                  backend=backend, motion=motion, **kw)
        t.init(vs, vt, R0)
        outs = []
        for _ in range(3):
            backend.calls.clear()
            o = t.step(vs, vt)
            outs.append([getattr(o, f).clone() for f in FIELDS])
            assert backend.calls == (WALK_CALLS if motion == "walk" else CV_CALLS)
        return outs

    a = run(cv.make_backend(ahv, oracle))                  # a backend without the two new ops
    b = run(ar.make_backend(ahv, oracle), adapt=None)
    assert all(torch.equal(x, y) for s, u in zip(a, b) for x, y in zip(s, u))


def _fp32_degrees(near):
    """Degrees d near ``near`` whose math.radians(d) is an fp32 number: the numpy backend scales its noise by math.radians(sigma)
    in fp64 and the record holds fp32 radians; for such a d the two are the same number."""
    x = np.float32(math.radians(near))
    for _ in range(64):
        d = math.degrees(float(x))
        if math.radians(d) == float(x):
            return d
        x = np.nextafter(x, np.float32(1))
    raise AssertionError("no fp32 radians near %r degrees" % near)


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_constant_rule_equals_the_fixed_tracker_bit_for_bit(ahv, oracle, g128, motion):
    """sigma_min = sigma_max = sigma and n_fresh_lost = n_fresh: the record never changes, and every TrackStep field of six steps
    (B = 2) is the fixed tracker's, bit for bit.  sigma and sigma_vel are degrees whose radians are fp32 numbers (_fp32_degrees)."""
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(2)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(40, seed=5))
    sigma, sigma_vel, F = _fp32_degrees(4.0), _fp32_degrees(1.5), 5
    assert abs(sigma - 4.0) < 1e-4 and abs(sigma_vel - 1.5) < 1e-4

    def run(**kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=24, sigma_deg=sigma, n_fresh=F, temperature=0.05, batch=2, seed=3,
                                  backend=ar.make_backend(ahv, oracle), motion=motion, sigma_vel_deg=sigma_vel, damping=0.9, **kw)
        t.init(vs, vt, R0)
        outs = []
        for _ in range(6):
            o = t.step(vs, vt)
            outs.append([getattr(o, f).clone() for f in FIELDS] + ([t.velocities.clone()] if motion != "walk" else []))
            if kw:
                d = ar.unpack(t.control_record.numpy())
                assert (d["sigma"] == np.float32(math.radians(sigma))).all() and (d["n_fresh"] == F).all()
                assert (d["sigma_vel"] == np.float32(math.radians(sigma_vel) if motion != "walk" else 0.0)).all()
        return outs

    fixed = run()
    adapted = run(adapt=ahv.track.AdaptiveNoise(sigma_min_deg=sigma, sigma_max_deg=sigma, score_floor=0.5, n_fresh_lost=F))
    for k, (s, u) in enumerate(zip(fixed, adapted)):
        for name, x, y in zip(FIELDS + ("velocities",), s, u):
            assert x.dtype == y.dtype and torch.equal(x, y), (k, name)


def test_track_sequence_forwards_adapt(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    item = next(iter(ahv.harness.SyntheticSequences(n_seq=1, n_frames=5, seed=3)))
    vols = {}

    class Model:
        def forward_features(self, a, b):
            f = lambda x: vols.setdefault(float(x.flatten()[0]), torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return f(a), f(b)

    rule = ahv.track.AdaptiveNoise()
    props = torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9))
    t = ahv.track.PoseTracker(W1, W2, b2, particles=16, n_fresh=2, batch=1, seed=1, backend=ar.make_backend(ahv, oracle), adapt=rule)
    res = ahv.harness.track_sequence(Model(), item, t, ref=0, proposals=props, device="cpu", adapt=ahv.track.AdaptiveNoise())
    c = res["control"]
    assert res["frames"] == [1, 2, 3, 4] and all(tuple(c[k].shape) == (4,) for k in ahv.ops.TrackControl._fields)
    assert float(c["sigma_deg"][0]) == pytest.approx(3.0) and torch.isnan(c["score"][0])              # the init frame: the fresh record
    assert torch.equal(c["score"][1:], res["score"][1:]) and float(c["sigma_deg"][-1]) == float(t.control().sigma_deg[0])
    with pytest.raises(RuntimeError, match="differs"):
        ahv.harness.track_sequence(Model(), item, t, ref=0, proposals=props, device="cpu", adapt=ahv.track.AdaptiveNoise(gain=2.0))
    plain = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=ar.make_backend(ahv, oracle))
    with pytest.raises(RuntimeError, match="built with adapt"):
        ahv.harness.track_sequence(Model(), item, plain, ref=0, proposals=props, device="cpu", adapt=True)
    assert "control" not in ahv.harness.track_sequence(Model(), item, plain, ref=0, proposals=props, device="cpu")


# ---- 4. the cases of the control kernel are what they claim ------------------------------------------------------------------
def test_control_cases_cover_the_classes_and_keep_off_the_thresholds(ahv):
    cases = ar.control_cases(ahv.rotations)
    assert sorted({c["B"] for c in cases}) == [1, 3, 180, 257] and {(c["M"], c["p"].first) for c in cases} == {(40, 1), (40, 2), (1, 1), (2, 2)}
    assert {c["V"] is not None for c in cases} == {False, True}
    angles, slots, scores, clamps, seen_nan_row = set(), set(), set(), set(), False
    for c in cases:
        p = c["p"]
        ref = ar.control(c["rec"], c["R"], c["V"], c["idx"], c["score"], p)
        angles.update(c["angle"].tolist())
        slots.update(c["slot"].tolist())
        scores.update(c["score_class"].tolist())
        seen_nan_row |= bool(c["nan_row"].any())
        assert np.isnan(ref["a"][c["nan_row"]]).all() and not ref["updated"][c["nan_row"]].any()
        # scores: the floor itself and the next float below it are the deliberate ones, every other score is far from it
        s, k = c["score"], c["score_class"]
        assert (s[k == 1] == np.float32(ar.FLOOR)).all() and not ref["lost"][k == 1].any()
        assert (s[k == 2] == np.nextafter(np.float32(ar.FLOOR), np.float32(-1))).all() and ref["lost"][k == 2].all()
        assert ref["lost"][k == 3].all() and not ref["lost"][k == 4].any() and not ref["lost"][k == 0].any()
        other = np.isfinite(s) & (k != 1) & (k != 2)
        assert (np.abs(s[other] - ar.FLOOR) > ar.NEAR).all()
        # slots: exactly at and one below max(M - nf, first), -1 and M
        at, under = c["slot"] == 1, c["slot"] == 2
        assert (c["idx"][at] == c["thr"][at]).all() and ref["reacquired"][at].all()
        assert (c["idx"][under] == c["thr"][under] - 1).all() and not ref["reacquired"][under].any()
        assert (c["idx"][c["slot"] == 3] == -1).all() and (c["idx"][c["slot"] == 4] == c["M"]).all()
        assert np.isnan(ref["a"][(c["slot"] == 3) | (c["slot"] == 4)]).all()
        assert not ref["reacquired"][c["slot"] == 3].any() and ref["reacquired"][c["slot"] == 4].all()
        # the innovations are the planted ones (fp32 rounding of the matrices aside)
        for cls, deg in enumerate(ar.ANGLES_DEG):
            sel = c["angle"] == cls
            if sel.any():
                assert np.abs(np.degrees(ref["a"][sel]) - deg).max() < 2e-5, (cls, deg)
                if c["V"] is None and deg == 0.0:
                    assert (ref["a"][sel] == 0.0).all()      # the winner is slot 0's bytes: exactly no innovation
        # sigma: no unclamped value within NEAR (relative) of a clamp, and all three outcomes occur
        free = ~ref["lost"]
        for bound in (p.sigma_min, p.sigma_max):
            assert (np.abs(ref["raw"][free] / bound - 1.0) > ar.NEAR).all()
        clamps.update(ref["clamped"][free].tolist())
        assert (ref["sigma"][ref["lost"]] == p.sigma_max).all() and (ref["n_fresh"][ref["lost"]] == p.n_fresh_lost).all()
        assert (ref["n_fresh"][free] == p.n_fresh0).all()
    assert angles >= {0, 1, 2, 3} and slots == set(range(6)) and scores == set(range(5)) and clamps == {-1, 0, 1} and seen_nan_row


# ---- 5. the three sequences ----------------------------------------------------------------------------------------------------
def _trackers(ahv, oracle, g128, s, P, specs):
    """name -> (init_frame, step_frame, control) on sequence s of P; ``specs``: name -> (sigma_deg, adapt kwargs or None)."""
    W1, W2, b2 = _head(g128)
    vs = torch.from_numpy(np.ascontiguousarray(g128["vol_src"]))
    R0 = torch.from_numpy(tr.planted_init(ahv.rotations, s))
    out = {}
    for name, (sigma, adapt) in specs.items():
        t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=sigma, n_fresh=P["n_fresh"], temperature=P["temperature"],
                                  batch=1, seed=s, backend=ar.make_backend(ahv, oracle),
                                  adapt=None if adapt is None else ahv.track.AdaptiveNoise(**adapt))
        out[name] = (lambda vt, t=t: t.init(vs, vt, R0), lambda vt, t=t: t.step(vs, vt), t.control if adapt is not None else None)
    rotate = lambda R: torch.from_numpy(oracle.rotate_volume(vs.numpy(), R[None].astype(np.float32)))
    return out, rotate


def _show(P, s, err):
    for name, (e, sig) in err.items():
        print("%s s=%d %-8s err: %s" % (P["name"], s, name, " ".join("%.2f" % x for x in e)))
        if not np.isnan(sig).all():
            print("%s s=%d %-8s sigma: %s" % (P["name"], s, name, " ".join("%.2f" % x for x in sig)))


@pytest.mark.parametrize("s", [0, 1, 2])
def test_accel_sequence(ahv, oracle, g128, s):
    """(A) 8 x 1 degree, 2.5, 4, 5.5, 7, 8.5, then 8 x 9 degrees per frame: the adapted tracker's largest error over frames
    14-21 stays below the fixed sigma = 3 walk's median over the same frames.  Measured on the oracle backend with numpy noise
    (adapted late max / fixed late median, degrees): 4.01 / 12.61, 3.58 / 14.21 and 3.82 / 8.14 for s = 0, 1, 2."""
    P = ar.ACCEL
    trackers, rotate = _trackers(ahv, oracle, g128, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed3": (3.0, None)})
    err = ar.run(ahv.rotations, s, P, rotate, trackers)
    _show(P, s, err)
    worst, median = ar.accel_bar(err["adapted"][0], err["fixed3"][0])
    print("ACCEL s=%d: adapted late max %.3f | fixed sigma 3 late median %.3f" % (s, worst, median))
    assert worst < median


@pytest.mark.parametrize("s", [0, 1, 2])
def test_settle_sequence(ahv, oracle, g128, s):
    """(B) 8 x 6 degrees, then 10 x 0.5 degrees per frame: the adapted tracker's mean error over frames 11-18 stays below the
    fixed sigma = 6 walk's, and it is never above 5 degrees after frame 2.  Measured on the oracle backend with numpy noise
    (adapted late mean / fixed sigma 6 late mean / adapted max after frame 2, degrees): 0.42 / 1.04 / 2.20, 0.49 / 0.97 / 2.66 and 0.35 / 1.12 / 2.23 for s = 0, 1, 2."""
    P = ar.SETTLE
    trackers, rotate = _trackers(ahv, oracle, g128, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed6": (6.0, None)})
    err = ar.run(ahv.rotations, s, P, rotate, trackers)
    _show(P, s, err)
    mean, mean6, worst = ar.settle_bar(err["adapted"][0], err["fixed6"][0])
    print("SETTLE s=%d: adapted late mean %.3f | fixed sigma 6 late mean %.3f | adapted max after frame 2 %.3f" % (s, mean, mean6, worst))
    assert mean < mean6
    assert worst <= 5.0


@pytest.fixture(scope="module")
def jump_runs(ahv, oracle, g128):
    runs = {}
    for s in (0, 1, 2):
        P = ar.JUMP
        trackers, rotate = _trackers(ahv, oracle, g128, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed3": (3.0, None)})
        runs[s] = ar.run(ahv.rotations, s, P, rotate, trackers)
    return runs


@pytest.mark.parametrize("s", [0, 1, 2])
def test_jump_sequence(jump_runs, s):
    """(C) 8 x 1 degree, one step of 70 degrees, 14 x 1 degree, score floor 0.8 and 128 fresh slots when lost: the adapted
    tracker's error is below 5 degrees on every frame 14-23.  Measured on the oracle backend with numpy noise (adapted late max /
    fixed sigma 3 late max, degrees): 1.95 / 113.98, 1.22 / 17.32 and 1.52 / 1.38 for s = 0, 1, 2 (the fixed tracker never recovers on s = 0 and
    is still off on s = 1)."""
    err = jump_runs[s]
    _show(ar.JUMP, s, err)
    worst, fixed = ar.jump_bar(err["adapted"][0], err["fixed3"][0])
    print("JUMP s=%d: adapted late max %.3f | fixed sigma 3, 16 fresh late max %.3f" % (s, worst, fixed))
    assert worst < ar.JUMP_BAR_DEG


def test_jump_sequence_defeats_the_fixed_tracker(jump_runs):
    """The fixed sigma = 3, 16-fresh tracker misses the 5 degree bar of (C) on at least one of the three sequences: the bar of
    test_jump_sequence is not one any tracker meets."""
    fixed = [ar.jump_bar(jump_runs[s]["adapted"][0], jump_runs[s]["fixed3"][0])[1] for s in (0, 1, 2)]
    print("JUMP: fixed sigma 3, 16 fresh late max %s" % " ".join("%.3f" % x for x in fixed))
    assert max(fixed) >= ar.JUMP_BAR_DEG
