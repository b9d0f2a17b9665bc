"""Noise scale and fresh slots adapted on the device: ``ahv_predict_rotations_ctl_f32`` bit for bit against the two plain
predict entry points, ``ahv_track_control_f32`` against the fp64 rule (tests/track_adapt_reference.py), the captured adaptive
step against the eager one, and the three planted sequences on the device's own noise.

Shapes: predict at M in {1, 2, 255, 256, 257} (no coast slot, no ordinary slot, the block edge, two blocks) and B in {1, 3};
control at B in {1, 3, 180, 257} (257: the first B past one workgroup of samples) and M in {40, 1, 2}.

Figures measured on the MI355X (this file prints them; DESIGN 4.2 quotes them):
  control against fp64, e_got / e_ref per innovation class (slot 0 wins, 0, 1e-3, 1, 170 degrees): a 0.90, 1.41, 0.59,
  0.59, 1.00 (and exactly 0 where the winner holds slot 0's bytes and there is no V); m 1.09, 1.00, 1.00, 1.39, 1.01; sigma 1.17, 0.30, 1.00, 1.41, 1.00; sigma_vel 1.15, 0.33, 1.00, 1.40, 1.00 (bar 4);
  largest e_got: a 6.0e-07 rad, m 1.7e-07 rad^2, sigma 9.3e-08 rad
  ACCEL, adapted max over frames 14-21 / fixed sigma 3 median: 6.06 / 10.83, 3.63 / 11.04, 3.91 / 10.21 degrees
  SETTLE, adapted mean over frames 11-18 / fixed sigma 6 mean / adapted max after frame 2: 0.45 / 1.08 / 2.53, 0.42 / 1.08 / 2.13,
  0.56 / 1.84 / 2.89 degrees
  JUMP, adapted max over frames 14-23 / fixed sigma 3, 16 fresh: 1.59 / 9.32, 2.18 / 71.88, 2.22 / 78.21 degrees
"""
import itertools
import math

import numpy as np
import pytest
import torch

from . import track_adapt_reference as ar
from . import track_reference as tr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
SEED, STEP = 0x1234ABCD5678, 5
MARGIN = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bytes_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the predict step, bit for bit ----------------------------------------------------------------------------------------
SIGMAS_DEG = (3.0, 0.7, 11.0)
SIGMA_VELS_DEG = (1.0, 0.0, 2.5)


def _fresh_values(M, k):
    """n_fresh of the samples of configuration k: -1, 0, M and M + 5 (clamped by the reader) and an ordinary value, rotated."""
    opts = (-1, 0, M, M + 5, min(2, M))
    return [opts[(k + b) % len(opts)] for b in range(3)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [1, 2, 255, 256, 257])
def test_predict_follows_the_record_bit_for_bit(ahv, ops, dev, B, M):
    """Row b of the controlled call is row b of the plain entry point called with the SAME B and sample b's sigma, sigma_vel and
    clamped n_fresh -- with and without idx, best_key, coast, V and both limits -- and the walk configuration is
    ``diffuse_rotations``."""
    N = 7
    R = _t(ahv.rotations.haar_rotations_np(B * N, seed=100 + M).reshape(B, N, 3, 3)).to(dev)
    V = _t((math.radians(5.0) * np.random.RandomState(M).standard_normal((B, N, 3))).astype(np.float32)).to(dev)
    idx = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(M), dtype=torch.int64)
    idx[0, 0] = -1
    idx[-1, -1] = N
    idx = idx.to(dev)
    keys = _t(ahv.dist.pack_keys_host(np.full(B, 0.5, np.float32), np.arange(B, dtype=np.int64) % N)).to(dev)
    step = torch.full((1,), STEP, dtype=torch.int64, device=dev)
    seen_fresh = set()
    for k, (use_idx, keyed, coast, use_V, limits) in enumerate(itertools.product((True, False), repeat=5)):
        nfs = _fresh_values(M, k)[:B]
        seen_fresh.update(nfs)
        sig = [SIGMAS_DEG[(k + b) % 3] for b in range(B)]
        sigv = [SIGMA_VELS_DEG[(k + 2 * b) % 3] for b in range(B)]
        rec = _t(ar.pack([ar.rad32(x) for x in sig], [ar.rad32(x) for x in sigv], nfs, 0, 1e-3, np.nan, np.nan)).to(dev)
        kw = dict(idx=idx if use_idx else None, m=None if use_idx else M, step=step, seed=SEED, best_key=keys if keyed else None,
                  max_angle_deg=2.0 if limits else None)
        cvkw = dict(kw, damping=0.9, coast=coast, max_speed_deg=4.0 if limits else None)
        out, vel, om = ops.predict_rotations_controlled(R, rec, V if use_V else None, want_omega=True, **cvkw)
        for b in range(B):
            nf = min(max(nfs[b], 0), M)
            ref = ops.predict_rotations(R, V if use_V else None, sigma_deg=sig[b], sigma_vel_deg=sigv[b], n_fresh=nf, want_omega=True, **cvkw)
            for name, x, y in zip(("out", "vel_out", "omega"), (out, vel, om), ref):
                assert _bytes_equal(x[b], y[b]), (name, b, nfs[b], use_idx, keyed, coast, use_V, limits)
        if coast or use_V:
            continue
        # the walk: no V, no coast slot, no vel_out
        got, gom = ops.predict_rotations_controlled(R, rec, velocities=False, want_omega=True, **kw)
        for b in range(B):
            nf = min(max(nfs[b], 0), M)
            ref = ops.diffuse_rotations(R, sigma_deg=sig[b], n_fresh=nf, want_omega=True, **kw)
            assert _bytes_equal(got[b], ref[0][b]) and _bytes_equal(gom[b], ref[1][b]), ("walk", b, nfs[b], use_idx, keyed, limits)
    assert seen_fresh >= {-1, 0, M, M + 5}
    # the record is read, not the launch: the same call after the record changed gives other bytes in sample 0 alone
    rec = _t(ar.pack([ar.rad32(3.0)] * B, 0.0, 0, 0, 1e-3, np.nan, np.nan)).to(dev)
    a = ops.predict_rotations_controlled(R, rec, idx=idx, step=step, seed=SEED, velocities=False).clone()
    rec[0, 0] = int(np.float32(ar.rad32(6.0)).view(np.int32))
    b_ = ops.predict_rotations_controlled(R, rec, idx=idx, step=step, seed=SEED, velocities=False)
    assert not _bytes_equal(a[0], b_[0]) and _bytes_equal(a[1:], b_[1:])


def test_ops_refuse_bad_device_arguments(ahv, ops, dev):
    B, M, N = 2, 6, 5
    R = _t(ahv.rotations.haar_rotations_np(B * N, seed=1).reshape(B, N, 3, 3)).to(dev)
    rec = ops.track_control_state(B, 3.0, 1.0, 2, dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    idx = torch.zeros((B, M), dtype=torch.int64, device=dev)
    for kw, word in ((dict(control=rec[:1]), "control must be"), (dict(control=rec.float()), "control must be"),
                     (dict(control=rec.cpu()), "control must be"), (dict(velocities=False, coast=True), "random walk"),
                     (dict(velocities=False, V=torch.zeros(B, N, 3, device=dev)), "random walk"),
                     (dict(velocities=False, vel_out=torch.zeros(B, M, 3, device=dev)), "random walk"), (dict(damping=1.5), "damping")):
        with pytest.raises(RuntimeError, match=word):
            ops.predict_rotations_controlled(R, **dict(dict(control=rec, idx=idx, step=step), **kw))
    P = _t(ahv.rotations.haar_rotations_np(B * M, seed=2).reshape(B, M, 3, 3)).to(dev)
    win, score = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, device=dev)
    for kw, word in ((dict(control=rec[:1]), "control must be"), (dict(idx=win.int()), "idx must be"), (dict(score=score[:1]), "score must be"),
                     (dict(V=torch.zeros(B, M, 4, device=dev)), "V must be"), (dict(first=3), "first"), (dict(sigma_deg=0.0), "sigma_deg"),
                     (dict(sigma_min_deg=9.0), "sigma_min"), (dict(gain=0.0), "gain"), (dict(rate=0.0), "rate"),
                     (dict(score_floor=float("nan")), "score_floor"), (dict(n_fresh=M + 1), "n_fresh"), (dict(n_fresh_lost=M + 1), "n_fresh_lost"),
                     (dict(reacquired=torch.zeros(B, device=dev)), "reacquired must be")):
        a = dict(dict(control=rec, R=P, idx=win, score=score), **kw)
        with pytest.raises(RuntimeError, match=word):
            ops.track_control(a.pop("control"), a.pop("R"), a.pop("idx"), a.pop("score"), **a)
    assert np.array_equal(rec.cpu().numpy(), ar.fresh_record(B, 3.0, 1.0, 2))          # no refused call touched the record


# ---- 2. the control step against the fp64 rule --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def control_runs(ahv, ops, dev):
    """Every case once: (case, fp64 reference, stock fp32, the device's record as a dict, its reacquired)."""
    runs = []
    for c in ar.control_cases(ahv.rotations):
        p = c["p"]
        rec = _t(c["rec"]).to(dev)
        reacq = ops.track_control(rec, _t(c["R"]).to(dev), _t(c["idx"]).to(dev), _t(c["score"]).to(dev),
                                  V=None if c["V"] is None else _t(c["V"]).to(dev), first=p.first, sigma_deg=3.0,
                                  sigma_vel_deg=1.0 if c["V"] is not None else 0.0, n_fresh=p.n_fresh0, sigma_min_deg=0.5,
                                  sigma_max_deg=8.0, gain=p.gain, rate=p.rate, score_floor=ar.FLOOR, n_fresh_lost=p.n_fresh_lost)
        args = (c["rec"], c["R"], c["V"], c["idx"], c["score"], p)
        raw = rec.cpu().numpy()
        assert (raw[:, 7] == 0).all()
        runs.append((c, ar.control(*args), ar.control_stock32(*args), ar.unpack(raw), reacq.cpu().numpy()))
    return runs


def test_control_decisions_are_exact(control_runs):
    """Flags, n_fresh, reacquired, the recorded score, every clamped sigma, an m that is not updated and a NaN innovation: exact."""
    for c, ref, _, got, reacq in control_runs:
        p, what = c["p"], (c["B"], c["M"])
        assert reacq.dtype == np.bool_ and np.array_equal(reacq, ref["reacquired"]), what
        assert np.array_equal(got["flags"], ref["flags"]), what
        assert np.array_equal(got["n_fresh"], ref["n_fresh"]), what
        assert np.array_equal(got["score"].view(np.uint32)[~np.isnan(c["score"])], c["score"].view(np.uint32)[~np.isnan(c["score"])]), what
        assert np.isnan(got["score"][np.isnan(c["score"])]).all(), what
        assert np.array_equal(np.isnan(got["a"]), np.isnan(ref["a"])), what
        low, high = ref["clamped"] == -1, ref["clamped"] == 1
        assert (got["sigma"][low] == np.float32(p.sigma_min)).all() and (got["sigma"][high] == np.float32(p.sigma_max)).all(), what
        for sel, bound in ((low, p.sigma_min), (high, p.sigma_max)):      # sigma_vel0 (sigma / sigma0) in fp32, both correctly rounded
            want = np.float32(p.sigma_vel0) * (np.float32(bound) / np.float32(p.sigma0))
            assert (got["sigma_vel"][sel] == want).all(), what
        keep = ~ref["updated"]
        assert np.array_equal(got["m"][keep].view(np.uint32), ar.unpack(c["rec"])["m"][keep].view(np.uint32)), what
        if c["V"] is None:      # the winner holds slot 0's bytes: exactly no innovation
            zero = c["angle"] == 0
            assert (got["a"][zero] == 0.0).all(), what


def test_control_values_match_fp64(control_runs):
    """sigma, sigma_vel (unclamped), m (updated) and the innovation a, per innovation class over all cases: e_got <= 4 e_ref, e_ref
    the error against fp64 of the same formula in stock fp32 torch on the CPU (tests/oplevel_cases.py's rule); where the stock
    formula is exact (e_ref = 0: an innovation of exactly 0, m' = m / 2) the kernel must be too."""
    groups = {}
    for c, ref, stock, got, _ in control_runs:
        free = ref["clamped"] == 0
        sel = dict(a=np.isfinite(ref["a"]), m=ref["updated"], sigma=free, sigma_vel=free & (c["p"].sigma_vel0 > 0))
        for name, where in sel.items():
            for cls in (-1, 0, 1, 2, 3):
                w = where & (c["angle"] == cls)
                if w.any():
                    g = groups.setdefault((name, cls), [0.0, 0.0, 0])
                    g[0] = max(g[0], float(np.abs(got[name][w].astype(np.float64) - ref[name][w]).max()))
                    g[1] = max(g[1], float(np.abs(stock[name].double().numpy()[w] - ref[name][w]).max()))
                    g[2] += int(w.sum())
    assert {k[0] for k in groups} == {"a", "m", "sigma", "sigma_vel"} and {k[1] for k in groups if k[0] == "a"} == {-1, 0, 1, 2, 3}
    bad = []
    for (name, cls), (e_got, e_ref, n) in sorted(groups.items()):
        label = "winner is slot 0" if cls < 0 else "innovation %g deg" % ar.ANGLES_DEG[cls]
        print("control %-9s %-22s n %4d  e_got %.3e  e_ref %.3e  e_got/e_ref %s"
              % (name, label, n, e_got, e_ref, "%.2f" % (e_got / e_ref) if e_ref > 0 else "-"))
        if not e_got <= MARGIN * e_ref:
            bad.append((name, label, e_got, e_ref))
    assert not bad, bad


# ---- 3. the captured step ------------------------------------------------------------------------------------------------------
def _planted(ahv, ops, dev, s, P, specs, **extra):
    h = load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    vs = _t(h["vol_src"]).to(dev)
    R0 = _t(tr.planted_init(ahv.rotations, s)).to(dev)
    trackers = {}
    for name, (sigma, adapt, kw) in specs.items():
        t = ahv.track.PoseTracker(*w, particles=P["particles"], sigma_deg=sigma, n_fresh=P["n_fresh"], temperature=P["temperature"],
                                  batch=1, seed=s, adapt=None if adapt is None else ahv.track.AdaptiveNoise(**adapt), **dict(extra, **kw))
        trackers[name] = (t, lambda vt, t=t: t.init(vs, vt, R0), lambda vt, t=t: t.step(vs, vt))
    rotate = lambda R: ops.rotate_volume(vs, _t(R[None].astype(np.float32)).to(dev))
    return trackers, rotate


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_captured_adaptive_steps_equal_eager_steps(ahv, ops, dev, motion):
    """JUMP's first 12 frames (init and 11 steps; the 70 degree step is the ninth, so the track is lost inside the replayed
    graphs and the last three steps run with sigma_max and n_fresh_lost): every TrackStep field and the record after every step are the eager tracker's, bit for bit -- sigma and
    n_fresh are read on the device at replay."""
    P, s = ar.JUMP, 0
    trackers, rotate = _planted(ahv, ops, dev, s, P, {"eager": (3.0, P["adapt"], {}), "graph": (3.0, P["adapt"], dict(use_graph=True))},
                                motion=motion)
    gt = ar.truth(ahv.rotations, s, P)
    lost, fresh = [], set()
    for k in range(12):
        vt = rotate(gt[k])
        res = {}
        for name, (t, init_frame, step_frame) in trackers.items():
            o = init_frame(vt) if k == 0 else step_frame(vt)
            res[name] = ([x.clone() for x in o if isinstance(x, torch.Tensor)], t.control_record.clone(),
                         None if t.velocities is None else t.velocities.clone())
        (a, ra, va), (b, rb, vb) = res["eager"], res["graph"]
        assert len(a) == len(b) and all(x.dtype == y.dtype and _bytes_equal(x.float(), y.float()) for x, y in zip(a, b)), k
        assert torch.equal(ra, rb), k
        assert (va is None and vb is None) or _bytes_equal(va, vb), k
        d = ops.decode_track_control(rb)
        lost.append(bool(d.lost[0]))
        fresh.add(int(d.n_fresh[0]))
    print("captured %s: lost per frame %s" % (motion, "".join("L" if x else "." for x in lost)))
    assert any(lost[3:]) and not all(lost[3:]) and fresh == {P["n_fresh"], P["adapt"]["n_fresh_lost"]}      # a lost episode, replayed


# ---- 4. the three sequences on the device's own noise ---------------------------------------------------------------------------
def _run(ahv, ops, dev, s, P, specs):
    trackers, rotate = _planted(ahv, ops, dev, s, P, {k: v + ({},) for k, v in specs.items()})
    entries = {name: (i, st, (t.control if t.adapt is not None else None)) for name, (t, i, st) in trackers.items()}
    err = ar.run(ahv.rotations, s, P, rotate, entries)
    for name, (e, sig) in err.items():
        print("%s s=%d on the device, %-8s err: %s" % (P["name"], s, name, " ".join("%.2f" % x for x in e)))
        if not np.isnan(sig).all():
            print("%s s=%d on the device, %-8s sigma: %s" % (P["name"], s, name, " ".join("%.2f" % x for x in sig)))
    return err


@pytest.mark.parametrize("s", [0, 1, 2])
def test_accel_sequence_on_the_device(ahv, ops, dev, s):
    P = ar.ACCEL
    err = _run(ahv, ops, dev, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed3": (3.0, None)})
    worst, median = ar.accel_bar(err["adapted"][0], err["fixed3"][0])
    print("ACCEL s=%d on the device: adapted late max %.3f | fixed sigma 3 late median %.3f" % (s, worst, median))
    assert worst < median


@pytest.mark.parametrize("s", [0, 1, 2])
def test_settle_sequence_on_the_device(ahv, ops, dev, s):
    P = ar.SETTLE
    err = _run(ahv, ops, dev, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed6": (6.0, None)})
    mean, mean6, worst = ar.settle_bar(err["adapted"][0], err["fixed6"][0])
    print("SETTLE s=%d on the device: adapted late mean %.3f | fixed sigma 6 late mean %.3f | adapted max after frame 2 %.3f"
          % (s, mean, mean6, worst))
    assert mean < mean6
    assert worst <= 5.0


@pytest.fixture(scope="module")
def jump_runs(ahv, ops, dev):
    P = ar.JUMP
    return {s: _run(ahv, ops, dev, s, P, {"adapted": (P["sigma_deg"], P["adapt"]), "fixed3": (3.0, None)}) for s in (0, 1, 2)}


@pytest.mark.parametrize("s", [0, 1, 2])
def test_jump_sequence_on_the_device(jump_runs, s):
    worst, fixed = ar.jump_bar(jump_runs[s]["adapted"][0], jump_runs[s]["fixed3"][0])
    print("JUMP s=%d on the device: adapted late max %.3f | fixed sigma 3, 16 fresh late max %.3f" % (s, worst, fixed))
    assert worst < ar.JUMP_BAR_DEG


def test_jump_sequence_defeats_the_fixed_tracker_on_the_device(jump_runs):
    fixed = [ar.jump_bar(jump_runs[s]["adapted"][0], jump_runs[s]["fixed3"][0])[1] for s in (0, 1, 2)]
    print("JUMP on the device: fixed sigma 3, 16 fresh late max %s" % " ".join("%.3f" % x for x in fixed))
    assert max(fixed) >= ar.JUMP_BAR_DEG
