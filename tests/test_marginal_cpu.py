"""Marginal smoothing, CPU tier: argument validation of ``ahv_marginal_step_f32`` / ``ahv_marginal_smooth_f32`` through the
ctypes table (validation runs before any HIP call), the host-side checks of the ops and of ``track.PoseTracker(marginals=True)``,
the fp64 reference (tests/marginal_reference.py) against brute-force marginals over every path, its closed forms, restart and
dead-frame rules, the control flow of the tracker on an oracle-backed backend, and the planted sequence with two distractor
frames."""
import math
import os
import re

import numpy as np
import pytest
import torch

from . import marginal_reference as mg
from . import posterior_reference as pr
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


def log_softmax(x):
    x = np.asarray(x, np.float64)
    return x - mg.lse(np.where(np.isfinite(x), x, -np.inf))


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


def test_marginal_step_argument_validation_needs_no_gpu(lib):
    # (0 R_cur, 1 scores, 2 step, 3 first_step, 4 B, 5 M, 6 H, 7 beta, 8 sigma, 9 jump, 10 hist_R, 11 hist_P, 12 hist_alpha,
    #  13 hist_emit, 14 stream)
    ok = [1, 1, 1, 1, 2, 8, 4, 50.0, 0.05, 8.0, 1, None, 1, 1, None]
    refused = _refuser(lib, lib.ahv_marginal_step_f32, ok, b"marginal_step")
    for slot in (0, 1, 2, 10, 12, 13):
        refused(b"null", **{"_%d" % slot: None})
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _5=bad)
    for bad in (0, -1, 65536):
        refused(b"B =", _4=bad)
    for bad in (1, 0, -2, 1 << 31):
        refused(b"H =", _6=bad)
    for bad in (0.0, -1.0, INF, float("nan")):
        refused(b"beta", _7=bad)
    for bad in (0.0, -0.1, INF, float("nan"), 1e-20):
        refused(b"sigma", _8=bad)
    for bad in (-0.5, float("nan"), -INF):
        refused(b"jump", _9=bad)


def test_marginal_smooth_argument_validation_needs_no_gpu(lib):
    # (0 hist_R, 1 hist_P, 2 hist_alpha, 3 hist_emit, 4 step, 5 first_step, 6 B, 7 M, 8 H, 9 F, 10 sigma, 11 jump, 12 logw, 13 idx,
    #  14 R, 15 stream)
    ok = [1, None, 1, 1, 1, 1, 2, 8, 4, 4, 0.05, 8.0, 1, 1, 1, None]
    refused = _refuser(lib, lib.ahv_marginal_smooth_f32, ok, b"marginal_smooth")
    for slot in (0, 2, 3, 4, 12, 13, 14):
        refused(b"null", **{"_%d" % slot: None})
    for bad in (0, -3, 1 << 31):
        refused(b"M =", _7=bad)
    for bad in (0, 65536):
        refused(b"B =", _6=bad)
    for bad in (1, 0, 1 << 31):
        refused(b"H =", _8=bad)
    for bad in (0, -1, 5):
        refused(b"F =", _9=bad)
    for bad in (0.0, -0.1, INF, float("nan"), 1e-20):
        refused(b"sigma", _10=bad)
    for bad in (-0.5, float("nan"), -INF):
        refused(b"jump", _11=bad)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n in (("ahv_marginal_step_f32", 15), ("ahv_marginal_smooth_f32", 16)):
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
            ops.marginal_history(2, 8, bad, "cpu")
    with pytest.raises(RuntimeError, match="B ="):
        ops.marginal_history(0, 8, 4, "cpu")
    with pytest.raises(RuntimeError, match="M ="):
        ops.marginal_history(2, 0, 4, "cpu")
    h, m = ops.smooth_history(2, 8, 4, "cpu"), ops.marginal_history(2, 8, 4, "cpu")
    assert isinstance(m, ops.MarginalHistory) and m._fields == ("alpha", "emit")
    assert tuple(m.alpha.shape) == tuple(m.emit.shape) == (4, 2, 8) and m.alpha.dtype == m.emit.dtype == torch.float32
    assert ops.SmoothedMarginals._fields == ("logw", "idx", "R")
    R, s, step = torch.eye(3).expand(2, 8, 3, 3).contiguous(), torch.zeros(2, 8), torch.ones(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.marginal_step(h, m, R, s, step, 0.02, 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.marginal_smooth(h, m, step, 3.0)
    with pytest.raises(RuntimeError, match="MarginalHistory"):
        ops.marginal_step(h, (m.alpha, m.emit), R, s, step, 0.02, 3.0)
    with pytest.raises(RuntimeError, match="MarginalHistory"):
        ops.marginal_smooth(h, None, step, 3.0)
    with pytest.raises(RuntimeError, match="SmoothHistory"):
        ops.marginal_step(None, m, R, s, step, 0.02, 3.0)
    with pytest.raises(RuntimeError, match="SmoothHistory"):
        ops.marginal_smooth((h.R, None, h.delta, h.back), m, step, 3.0)


def test_tracker_constructor_checks(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    T = ahv.track.PoseTracker
    with pytest.raises(RuntimeError, match="marginals=True needs history"):
        T(W1, W2, b2, particles=8, marginals=True, backend=mg.make_backend(ahv, oracle))
    with pytest.raises(RuntimeError, match="marginal_step"):
        T(W1, W2, b2, particles=8, history=4, marginals=True, backend=sm.make_backend(ahv, oracle))   # a backend without the ops
    t = T(W1, W2, b2, particles=8, history=4, backend=sm.make_backend(ahv, oracle))                    # ... is fine without them
    assert t.marginals is False and t._marg is None
    with pytest.raises(RuntimeError, match="marginals=True"):
        t.smoothed_marginals()
    t = T(W1, W2, b2, particles=8, batch=2, history=4, marginals=True, backend=mg.make_backend(ahv, oracle))
    assert isinstance(t._marg, ahv.ops.MarginalHistory) and tuple(t._marg.alpha.shape) == (4, 2, 8)
    with pytest.raises(RuntimeError, match="before the first step"):
        t.smoothed_marginals()


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


def _run(Rs, scores, beta, sigma, jump, H, Vs=None, damping=1.0, B=1):
    """The recursions over every frame: (ring, marginal ring).  The marginal step of a frame runs BEFORE the ring records it on
    even frames and after it on odd ones: it reads the previous slot only."""
    ring = sm.Ring(H, B, len(scores[0]), velocities=Vs is not None)
    mr = mg.MarginalRing(ring)
    for f in range(len(scores)):
        rec = lambda: ring.step(f + 1, Rs[f][None], scores[f][None], beta, sigma, jump, V=None if Vs is None else Vs[f][None],
                                damping=damping)
        if f % 2:
            rec()
        mr.step(f + 1, Rs[f][None], scores[f][None], beta, sigma, jump)
        if not f % 2:
            rec()
    return ring, mr


@pytest.mark.parametrize("M,T", [(3, 4), (4, 3)])
@pytest.mark.parametrize("jump", [0.0, 2.0, 8.0, INF])
def test_reference_equals_brute_force(ahv, M, T, jump):
    for seed, sigma_deg, dead in ((1, 3.0, False), (2, 30.0, False), (3, 10.0, True)):
        Rs, scores = _tiny(ahv, M, T, seed, sigma_deg, dead)
        beta, sigma = 1.0 / 0.2, math.radians(sigma_deg)
        for H in (T, T + 1):
            ring, mr = _run(Rs, scores, beta, sigma, jump, H)
            logw, idx, Rp = mr.smooth(T, T, sigma, jump)
            want = mg.brute_force_marginals(Rs, Rs, scores, beta, sm.inv4s2(sigma), jump)
            for f in range(T):
                fin = np.isfinite(want[f])
                assert np.array_equal(np.isfinite(logw[0, f]), fin), (seed, f)
                assert np.abs(logw[0, f][fin] - want[f][fin]).max() < 1e-10, (seed, f)
                assert idx[0, f] == int(np.argmax(logw[0, f])) and np.array_equal(Rp[0, f], Rs[f][idx[0, f]])
                assert abs(np.exp(logw[0, f][fin]).sum() - 1.0) < 1e-12
            # a shorter window: the newest frames' marginals given those frames alone still sum to one
            short = mr.smooth(T, 2, sigma, jump)[0]
            assert np.abs(np.exp(short[0]).sum(axis=-1) - 1.0).max() < 1e-12


def test_reference_with_velocities_equals_brute_force(ahv):
    M, T, jump, damping = 3, 4, 8.0, 0.8
    Rs, scores = _tiny(ahv, M, T, 5, 5.0)
    rs = np.random.RandomState(9)
    Vs = [math.radians(6.0) * rs.standard_normal((M, 3)) for _ in range(T)]
    Ps = [sm.predicted(R, V, damping) for R, V in zip(Rs, Vs)]
    sigma = math.radians(5.0)
    ring, mr = _run(Rs, scores, 5.0, sigma, jump, T, Vs=Vs, damping=damping)             # H = T: every slot in use
    logw = mr.smooth(T, T, sigma, jump)[0]
    want = mg.brute_force_marginals(Rs, Ps, scores, 5.0, sm.inv4s2(sigma), jump)
    assert np.abs(logw[0] - np.stack(want)).max() < 1e-10
    # the predicted poses matter: without them the marginals are different numbers
    other = mg.brute_force_marginals(Rs, Rs, scores, 5.0, sm.inv4s2(sigma), jump)
    assert np.abs(np.stack(other) - np.stack(want)).max() > 1e-3


def test_jump_zero_is_the_per_frame_softmax(ahv):
    M, T = 4, 5
    for seed in (1, 2, 3):
        Rs, scores = _tiny(ahv, M, T, seed, 3.0, dead=seed == 3)
        ring, mr = _run(Rs, scores, 50.0, math.radians(3.0), 0.0, 3)                     # the ring wraps
        logw, idx, _ = mr.smooth(T, 3, math.radians(3.0), 0.0)
        for f in range(3):
            want = log_softmax(50.0 * np.where(np.isfinite(scores[T - 3 + f]), scores[T - 3 + f], -np.inf))
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(logw[0, f]), fin) and np.abs(logw[0, f][fin] - want[fin]).max() < 1e-12
            assert idx[0, f] == int(np.argmax(want))


def test_last_frame_is_the_softmax_of_alpha(ahv):
    M, T = 4, 5
    Rs, scores = _tiny(ahv, M, T, 6, 5.0, dead=True)
    sigma = math.radians(5.0)
    ring, mr = _run(Rs, scores, 5.0, sigma, 8.0, 6)
    for F in (1, 3, 5):
        logw = mr.smooth(T, F, sigma, 8.0)[0]
        want = log_softmax(mr.alpha[T % 6, 0])
        fin = np.isfinite(want)
        assert fin.sum() == M - 1 and np.array_equal(np.isfinite(logw[0, -1]), fin)
        assert np.abs(logw[0, -1][fin] - want[fin]).max() < 1e-12


def test_restart_and_dead_frame_rules(ahv):
    M, H = 3, 8
    Rs, scores = _tiny(ahv, M, 7, 4, 3.0)
    scores[3][:] = np.nan                                       # frame 4: every score non-finite
    scores[5][1] = np.inf                                       # frame 6: one dead particle
    Rs[1][2] = np.nan                                           # frame 2: a NaN pose -- no edge into it, none out of it
    sigma = math.radians(3.0)
    ring, mr = _run(Rs, scores, 5.0, sigma, 8.0, H)
    assert np.array_equal(mr.alpha[1, 0], 5.0 * scores[0]) and np.array_equal(mr.emit[1, 0], 5.0 * scores[0])
    assert mr.alpha[2, 0, 2] == -np.inf and mr.emit[2, 0, 2] == 5.0 * scores[1][2]        # alive, predecessors alive, no edge
    assert np.isfinite(mr.alpha[2, 0, :2]).all() and np.isfinite(mr.alpha[3, 0]).all()
    assert np.all(mr.alpha[4, 0] == -np.inf) and np.all(mr.emit[4, 0] == -np.inf)
    assert np.array_equal(mr.alpha[5, 0], 5.0 * scores[4])                                 # frame 5 restarts
    assert mr.alpha[6, 0, 1] == -np.inf and mr.emit[6, 0, 1] == -np.inf and np.isfinite(mr.alpha[6, 0, [0, 2]]).all()
    logw, idx, Rp = mr.smooth(7, 8, sigma, 8.0)                  # more frames than were recorded
    assert np.all(logw[0, 0] == -np.inf) and idx[0, 0] == -1 and np.array_equal(Rp[0, 0], np.eye(3))     # before first_step
    assert np.all(logw[0, 4] == -np.inf) and idx[0, 4] == -1 and np.array_equal(Rp[0, 4], np.eye(3))     # the dead frame
    assert logw[0, 2, 2] == -np.inf and logw[0, 6, 1] == -np.inf
    for f in (1, 2, 3, 5, 6, 7):
        fin = np.isfinite(logw[0, f])
        assert idx[0, f] >= 0 and abs(np.exp(logw[0, f][fin]).sum() - 1.0) < 1e-12
    # behind the dead frame beta is 0: frames 1-3 are the marginals of a sequence that ends at frame 3
    ring3, mr3 = _run(Rs[:3], scores[:3], 5.0, sigma, 8.0, H)
    assert np.array_equal(mr3.smooth(3, 3, sigma, 8.0)[0][0], logw[0, 1:4])
    # ... and frames 5-7 those of a sequence that starts at frame 5
    ring5 = sm.Ring(H, 1, M)
    mr5 = mg.MarginalRing(ring5)
    for f in (4, 5, 6):
        mr5.step(f + 1, Rs[f][None], scores[f][None], 5.0, sigma, 8.0, first_step=5)
        ring5.step(f + 1, Rs[f][None], scores[f][None], 5.0, sigma, 8.0, first_step=5)
    assert np.array_equal(mr5.smooth(7, 3, sigma, 8.0, first_step=5)[0][0], logw[0, 5:8])
    # a later first_step hides the older frames
    l2, i2, _ = mr.smooth(7, 8, sigma, 8.0, first_step=6)
    assert np.all(l2[0, :6] == -np.inf) and np.all(i2[0, :6] == -1) and np.isfinite(l2[0, 6:]).any(axis=-1).all()


# ---- 4. the control flow on the oracle backend -------------------------------------------------------------------------
@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_tracker_control_flow(ahv, oracle, g128, motion):
    W1, W2, b2 = _head(g128)
    B, M, N0, H = 2, 24, 40, 4
    vs, vt = _pair(B)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    calls = (WALK_CALLS if motion == "walk" else CV_CALLS) + ["smooth_step"]
    kw = dict(particles=M, sigma_deg=4.0, n_fresh=5, temperature=0.05, batch=B, seed=3, motion=motion, sigma_vel_deg=1.5, damping=0.9,
              history=H, mode_angle_deg=20.0)

    def run(marginals):
        be = mg.make_backend(ahv, oracle, cv.make_backend(ahv, oracle))
        t = ahv.track.PoseTracker(W1, W2, b2, backend=be, marginals=marginals, **kw)
        t.init(vs, vt, R0)
        assert "marginal_step" not in be.calls            # init records nothing
        outs, paths, margs = [], [], []
        for n in range(1, 7):
            be.calls.clear()
            o = t.step(vs, vt)
            assert be.calls == calls + (["marginal_step"] if marginals else []), be.calls      # right after smooth_step
            outs.append([x.clone() if isinstance(x, torch.Tensor) else x for x in o])
            p = t.smoothed()
            paths.append((p.idx.clone(), p.R.clone()))
            if marginals:
                lm = be.last_marginal
                assert lm["t"] == n and lm["first_step"] == 1 and lm["jump"] == 8.0
                assert abs(lm["sigma_deg"] - (4.0 if motion == "walk" else math.hypot(4.0, 1.5))) < 1e-12
                F = min(n, H)
                m = t.smoothed_marginals()
                assert tuple(m.logw.shape) == (B, F, M) and tuple(m.idx.shape) == (B, F) and tuple(m.R.shape) == (B, F, 3, 3)
                assert m.idx.dtype == torch.int64 and (m.idx >= 0).all()
                assert torch.allclose(m.logw.double().exp().sum(-1), torch.ones(B, F, dtype=torch.float64), atol=1e-5)
                assert tuple(t.smoothed_marginals(frames=2).logw.shape) == (B, min(n, 2), M)
                rows = torch.arange(B)
                assert torch.equal(m.R[:, -1], o.particles[rows, m.idx[:, -1]])              # a particle of this step
                # the newest frame's marginal is the filter's posterior: the log-softmax of alpha
                assert torch.allclose(m.logw[:, -1], torch.log_softmax(t._marg.alpha[n % H], dim=-1), atol=1e-5)
                out = ahv.ops.SmoothedMarginals(torch.empty(B, F, M), torch.empty(B, F, dtype=torch.int64), torch.empty(B, F, 3, 3))
                again = t.smoothed_marginals(out=out)
                assert again.logw.data_ptr() == out.logw.data_ptr() and torch.equal(out.logw, m.logw) and torch.equal(out.idx, m.idx)
                be.calls.clear()
                m2, R_mean, spread, mass, entropy = t.smoothed_marginals(posterior=True)
                assert be.calls == ["marginal_smooth", "pose_posterior"]
                assert torch.equal(m2.logw, m.logw) and tuple(R_mean.shape) == (B, F, 3, 3)
                assert tuple(spread.shape) == tuple(mass.shape) == tuple(entropy.shape) == (B, F)
                assert (mass > 0).all() and (mass <= 1 + 1e-6).all() and (entropy >= -1e-6).all()
                p_ = m.logw.double().exp()                                                    # the entropy of the stored row
                assert torch.allclose(entropy.double(), -(p_ * m.logw.double().clamp_min(-1e30)).sum(-1), atol=1e-4)
                # the mean pose is the projection of the weighted mean of the frame's recorded set
                slot = (n - F + 1) % H
                mean = torch.einsum("bm,bmij->bij", p_[:, 0], t._hist.R[slot].double())
                for b in range(B):
                    assert np.abs(R_mean[b, 0].double().numpy() - pr.nearest_rotation(mean[b].numpy())[0]).max() < 1e-5
                margs.append(m.logw.clone())
        return t, be, outs, paths, margs

    t0, _, plain, ppaths, _ = run(False)
    t1, be, with_m, mpaths, margs = run(True)
    for a, b in zip(plain, with_m):
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)         # the marginals observe, never steer
    for (ia, Ra), (ib, Rb) in zip(ppaths, mpaths):
        assert torch.equal(ia, ib) and torch.equal(Ra, Rb)
    for x, y in zip(t0._hist, t1._hist):
        assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a new init hides the old slots: after one more step the marginals have one frame, the softmax of its scores
    t1.init(vs, vt, R0)
    with pytest.raises(RuntimeError, match="before the first step"):
        t1.smoothed_marginals()
    o = t1.step(vs, vt)
    m = t1.smoothed_marginals()
    assert tuple(m.logw.shape) == (B, 1, M) and int(be.last_marginal["t"]) == 1
    assert torch.allclose(m.logw[:, 0], torch.log_softmax(o.scores / 0.05, dim=-1), atol=1e-5)


def test_track_sequence_marginals_keyword(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    item = next(iter(ahv.harness.SyntheticSequences(n_seq=1, n_frames=6, seed=3)))
    vols = {}

    class Model:
        def forward_features(self, a, b):
            f = lambda x: vols.setdefault(float(x.flatten()[0]), torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return f(a), f(b)

    props = torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9))
    mk = lambda **kw: ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=mg.make_backend(ahv, oracle), **kw)
    plain = ahv.harness.track_sequence(Model(), item, mk(), ref=0, proposals=props, device="cpu")
    assert sorted(plain) == ["R_map", "err", "frames", "score"]                    # the default result is unchanged
    both = ahv.harness.track_sequence(Model(), item, mk(history=3), ref=0, proposals=props, device="cpu", smoothed=True)
    res = ahv.harness.track_sequence(Model(), item, mk(history=3, marginals=True), ref=0, proposals=props, device="cpu", smoothed=True,
                                     marginals=True)
    for k in plain:
        assert (plain[k] == res[k]) if k == "frames" else torch.equal(plain[k], res[k])
    for k in both["smoothed"]:
        assert (both["smoothed"][k] == res["smoothed"][k]) if k == "frames" else torch.equal(both["smoothed"][k], res["smoothed"][k])
    m = res["marginals"]
    assert sorted(m) == sorted(["frames", "idx", "R", "err", "R_mean", "err_mean", "spread_deg", "mode_mass", "entropy"])
    assert m["frames"] == [3, 4, 5] and tuple(m["R"].shape) == tuple(m["R_mean"].shape) == (3, 3, 3) and tuple(m["idx"].shape) == (3,)
    for k in ("err", "err_mean", "spread_deg", "mode_mass", "entropy"):
        assert tuple(m[k].shape) == (3,), k
    for k, f in enumerate(m["frames"]):
        R_gt = item["R"][f] @ item["R"][0].T
        assert abs(float(m["err"][k]) - float(ahv.rotations.geodesic_deg(m["R"][k][None], R_gt[None]))) < 1e-4
        assert abs(float(m["err_mean"][k]) - float(ahv.rotations.geodesic_deg(m["R_mean"][k][None], R_gt[None]))) < 1e-4
    with pytest.raises(RuntimeError, match="marginals=True"):
        ahv.harness.track_sequence(Model(), item, mk(history=3), ref=0, proposals=props, device="cpu", marginals=True)


# ---- 5. the planted sequence with two distractor frames ----------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_distractor(ahv, oracle, g128, s):
    """smooth_reference.DISTRACTED (frames 5 and 8 replaced by an unrelated view; history 12, smoothing sigma 3 degrees, jump 8)
    on the oracle backend with numpy noise.  Judged over frames 4-11 against the blind 4 096-hypothesis median of the clean
    sequence: the arg-max of every frame's smoothed marginal and the marginal-weighted mean pose of ``posterior=True``.  Measured,
    degrees (arg-max / mean / blind median): 3.74 / 4.16 / 8.44, 3.15 / 3.54 / 8.00 and 3.18 / 2.94 / 7.01 for s = 0, 1, 2."""
    P = sm.DISTRACTED
    W1, W2, b2 = _head(g128)
    vs = torch.from_numpy(np.ascontiguousarray(g128["vol_src"]))
    R0 = torch.from_numpy(tr.planted_init(ahv.rotations, s))
    w = [x.numpy() for x in (W1, W2, b2)]
    t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                              temperature=P["temperature"], batch=1, seed=s, backend=mg.make_backend(ahv, oracle),
                              history=P["history"], smooth_sigma_deg=P["smooth_sigma_deg"], smooth_jump=P["smooth_jump"], marginals=True)
    rotate = lambda R: torch.from_numpy(oracle.rotate_volume(vs.numpy(), R[None].astype(np.float32)))
    got = {}

    def query():
        got["m"], got["R_mean"], got["spread"], got["mass"], got["entropy"] = t.smoothed_marginals(posterior=True)
        return got["m"]

    filt, arg_err = sm.distracted_run(ahv.rotations, s, rotate, lambda vt: t.init(vs, vt, R0), lambda vt: t.step(vs, vt), query)
    gt = tr.planted_truth(ahv.rotations, s)
    mean_err = tr.geodesic_deg(got["R_mean"][0].double().numpy(), gt[1:])
    blind = []
    for k in range(P["frames"]):
        vt = rotate(gt[k])
        Rb = R0.numpy()[int(oracle.score_hypotheses(vs.numpy(), vt.numpy(), R0.numpy(), *w)[2][0])]
        blind.append(float(tr.geodesic_deg(Rb.astype(np.float64), gt[k])))
    worst_arg, median = sm.distracted_bar(arg_err, blind)
    worst_mean, _ = sm.distracted_bar(mean_err, blind)
    print("distractor s=%d: filter %s | marginal arg-max (frames 1-11) %s | mean pose %s | max over 4-11: arg-max %.3f, mean %.3f | "
          "blind median %.3f | mode mass %s | spread %s"
          % (s, " ".join("%.2f" % e for e in filt), " ".join("%.2f" % e for e in arg_err), " ".join("%.2f" % e for e in mean_err),
             worst_arg, worst_mean, median, " ".join("%.2f" % e for e in got["mass"][0]), " ".join("%.2f" % e for e in got["spread"][0])))
    for k in P["distractors"]:
        assert filt[k] > 90.0, (k, filt[k])               # the premise: the filter follows the distractor
    assert worst_arg < median
    assert worst_mean < median
