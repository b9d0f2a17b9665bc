"""Constant-velocity pose tracking on the device: ``ahv_predict_rotations_f32`` against the fp64 reference
(tests/track_cv_reference.py), its slot classes, the noise it draws, its limits, and ``track.PoseTracker(motion=
"constant_velocity")`` (determinism, the captured step against the eager one, no drift, the fast planted sequence).

Shapes: B = 3; exact slots at M in {1, 2, 3, 257} (no coast slot, no ordinary slot, one ordinary slot, two blocks); parity at
N in {1, 5, 1025} and M in {2, 255, 256, 257, 1025} (the block edges, several blocks with a ragged end).

Figures measured on the MI355X (this file prints them; DESIGN 4.2 quotes them):
  rotations against fp64, max |entry| error over all cases: kernel 4.8e-07, stock fp32 torch composition 3.3e-07 (bar 4 x)
  velocities against fp64: kernel 1.5e-08, stock fp32 torch damping * v + noise 2.4e-08 (bar 4 x)
  without velocities against ops.diffuse_rotations: rotations 3.6e-07, omega identical (bar: 4 x the stock figure, 1.3e-06)
  noise, n = 36 864: ECDF gaps 0.0030-0.0061 (band 0.0140), |mean| <= 0.0061, |correlation| <= 0.0156 (bound 0.0260)
  no drift, max |R^T R - I| after 256 chained calls: 4.7e-07; ops.random_rotations output of the same size: 6.4e-07 (bar 4 x)
  fast planted sequence, constant-velocity max over frames 8-15 / walk median over the same frames: 1.83 / 98.40, 1.22 / 17.04,
  2.08 / 28.06 degrees
"""
import math

import numpy as np
import pytest
import torch

from . import track_cv_reference as cv
from . import track_reference as tr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
B = 3
SEED, STEP = 0x1234ABCD5678, 5
ALPHA = 1e-6


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


def _step(dev, value=STEP):
    return torch.full((1,), value, dtype=torch.int64, device=dev)


def _set(ahv, N, per_sample, seed=0):
    R = ahv.rotations.haar_rotations_np(B * N if per_sample else N, seed=100 + N + seed)
    return _t(R.reshape(B, N, 3, 3) if per_sample else R)


def _vel(N, per_sample, deg=5.0, seed=0):
    """Velocities (N,3) / (B,N,3) float32: Gaussian, ``deg`` degrees per component."""
    rs = np.random.RandomState(7 + N + seed)
    return _t((math.radians(deg) * rs.standard_normal((B, N, 3) if per_sample else (N, 3))).astype(np.float32))


def _idx(N, M, seed=0):
    return torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(N + M + seed), dtype=torch.int64)


def _keys(ahv, N, dev):
    """Sample 0: the valid index N - 1; sample 1: EMPTY; sample 2: an index outside [0, N).  The last two read row 0."""
    keys = ahv.dist.pack_keys_host(np.array([0.5, 0.0, 0.25], np.float32), np.array([N - 1, 0, N + 3], np.int64)).copy()
    keys[1] = ahv.dist.KEY_EMPTY
    return _t(keys).to(dev), np.array([N - 1, 0, 0])


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dkw(n):
    return math.sqrt(math.log(2.0 / ALPHA) / (2.0 * n))


def ecdf_gap(x, cdf):
    """sup |F_n - F| of the sample x against the continuous cdf."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    F = np.array([cdf(v) for v in x])
    return float(max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(0, n) / n)))


PHI = lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0)))
f32 = lambda x: float(np.float32(x))


# ---- 2. fp64 parity (first: its bar serves the other tests) ------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy(ahv, ops, dev):
    """Every case once: max |entry| error of the kernel's rotations, and of the stock fp32 torch composition, against
    R_i exp([omega]x) in fp64 with the omega the kernel reported; and max |entry| error of the kernel's velocities, and of the
    stock fp32 ``damping * v + noise``, against the same in fp64, with the noise the kernel reports when there is no V.
    idx holds -1 and N entries (row 0).  With a key, slot 0 is the elite and slot 1 coasts: both are held to the same figures."""
    rot = ahv.rotations
    kern = stock = kern_v = stock_v = 0.0
    noise = {}
    for sv in (0.0, 1.0):   # the velocity noise of a slot is a function of (seed, step, b, j): draw it once, at the largest M
        noise[sv] = ops.predict_rotations(_set(ahv, 1, False).to(dev), idx=torch.zeros((B, 1025), dtype=torch.int64, device=dev),
                                          sigma_deg=0.0, sigma_vel_deg=sv, step=_step(dev), seed=SEED)[1].cpu()
    for N in (1, 5, 1025):
        keys, best = _keys(ahv, N, dev)
        for vmode, per_sample in ((None, False), (None, True), ("shared", False), ("per", True)):
            R = _set(ahv, N, per_sample, seed=1)
            V = None if vmode is None else _vel(N, vmode == "per")
            Rd, Vd = R.to(dev), None if V is None else V.to(dev)
            for M in (2, 255, 256, 257, 1025):
                idx = _idx(N, M)
                idx[0, 0], idx[-1, -1] = -1, N
                if M > 2:
                    idx[1, 2] = N
                idx_d = idx.to(dev)
                for keyed in (False, True):
                    src = idx.numpy().copy()
                    if keyed:
                        src[:, 0] = src[:, 1] = best          # the rows the elite and the coast slot read
                    rows = _t(tr.gather(R.numpy(), src))
                    vrows = np.zeros((B, M, 3)) if V is None else cv.gather_vel(V.double().numpy(), src)
                    lo = 2 if keyed else 0
                    for sigma in (3.0, 30.0):
                        for sv in (0.0, 1.0):
                            for damping in (0.0, 0.9, 1.0):
                                out, vel, om = ops.predict_rotations(Rd, Vd, idx=idx_d, sigma_deg=sigma, sigma_vel_deg=sv,
                                                                     damping=damping, step=_step(dev), seed=SEED,
                                                                     best_key=keys if keyed else None, coast=True, want_omega=True)
                                out, vel, om = out.cpu(), vel.cpu(), om.cpu()
                                want = rows.double().numpy() @ tr.exp_so3(om.double().numpy())
                                kern = max(kern, float(np.abs(out.double().numpy() - want).max()))
                                E = rot.axis_angle_to_matrix(om.reshape(-1, 3)).reshape(B, M, 3, 3)          # fp32 on the CPU
                                stock = max(stock, float(np.abs(torch.matmul(rows, E).double().numpy() - want).max()))
                                if keyed:     # the elite's and the coast slot's velocity: the row's, bit for bit
                                    assert np.array_equal(vel[:, :2].double().numpy(), vrows[:, :2])
                                    assert not om[:, 0].any() and torch.equal(om[:, 1], vel[:, 1])
                                if M > lo:
                                    a = noise[sv][:, lo:M]
                                    want_v = f32(damping) * vrows[:, lo:] + a.double().numpy()
                                    kern_v = max(kern_v, float(np.abs(vel[:, lo:].double().numpy() - want_v).max()))
                                    st = torch.tensor(damping, dtype=torch.float32) * _t(vrows[:, lo:]).float() + a
                                    stock_v = max(stock_v, float(np.abs(st.double().numpy() - want_v).max()))
    return kern, stock, kern_v, stock_v


def test_predicted_slots_match_fp64(accuracy):
    kern, stock, kern_v, stock_v = accuracy
    print("predicted slots, max |entry| error against fp64: kernel %.3e, stock fp32 torch composition %.3e; velocities: kernel "
          "%.3e, stock fp32 torch %.3e" % (kern, stock, kern_v, stock_v))
    assert kern <= 4.0 * stock
    assert kern_v <= 4.0 * stock_v


# ---- 1. exact slots ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True])
def test_slot_classes_are_exact(ahv, ops, dev, accuracy, per_sample):
    bar = 4.0 * accuracy[1]
    for N in (1, 5):
        R, V = _set(ahv, N, per_sample), _vel(N, per_sample)
        Rd, Vd = R.to(dev), V.to(dev)
        keys, best = _keys(ahv, N, dev)
        elite_R, elite_V = _t(tr.gather(R.numpy(), best[:, None]))[:, 0], _t(cv.gather_vel(V.numpy(), best[:, None]))[:, 0]
        for M in (1, 2, 3, 257):
            idx = _idx(N, M).to(dev)
            for nf in sorted({0, min(2, M), M}):
                kw = dict(idx=idx, sigma_deg=3.0, step=_step(dev), seed=SEED, n_fresh=nf)
                ref = ops.diffuse_rotations(Rd, best_key=keys, **kw)
                for Vin, coast in ((Vd, True), (None, True), (Vd, False)):
                    out, vel, om = ops.predict_rotations(Rd, Vin, best_key=keys, coast=coast, want_omega=True, **kw)
                    what = (N, M, nf, Vin is not None, coast)
                    v_n = elite_V if Vin is not None else torch.zeros_like(elite_V)
                    # elite: R and v bit for bit (EMPTY and out-of-range keys read row 0), omega = 0
                    assert _bytes_equal(out[:, 0].cpu(), elite_R) and _bytes_equal(vel[:, 0].cpu(), v_n), what
                    assert not om[:, 0].any(), what
                    lo = 1
                    if coast and M >= 2:   # coast: slot 1 whatever n_fresh says; v kept, omega = v, R moved by exp([v]x)
                        lo = 2
                        assert _bytes_equal(vel[:, 1].cpu(), v_n) and _bytes_equal(om[:, 1].cpu(), v_n), what
                        want = elite_R.double().numpy() @ tr.exp_so3(v_n.double().numpy())
                        assert float(np.abs(out[:, 1].cpu().double().numpy() - want).max()) <= bar, what
                        if Vin is None:      # v = 0: the previous arg-max itself, within the fp64 bar
                            assert float((out[:, 1].cpu().double() - elite_R.double()).abs().max()) <= bar, what
                    # fresh: the bytes diffuse_rotations writes for the same arguments; v = omega = 0
                    lo = max(M - nf, lo)
                    assert _bytes_equal(out[:, lo:], ref[:, lo:]), what
                    assert not vel[:, lo:].any() and not om[:, lo:].any(), what
                    first = 2 if coast else 1
                    if lo > first:
                        assert om[:, first:lo].abs().sum(-1).min() > 0, what      # the ordinary slots did move
            # no key: no elite and no coast slot; with n_fresh = M every slot is fresh
            kw = dict(idx=idx, sigma_deg=3.0, step=_step(dev), seed=SEED, n_fresh=M)
            out, vel, om = ops.predict_rotations(Rd, Vd, coast=True, want_omega=True, **kw)
            assert _bytes_equal(out, ops.diffuse_rotations(Rd, **kw)) and not vel.any() and not om.any()


# ---- 3. reduction to diffuse_rotations -----------------------------------------------------------------------------------
def test_reduces_to_diffuse_rotations(ahv, ops, dev, accuracy):
    bar = 4.0 * accuracy[1]
    worst = worst_w = 0.0
    for per_sample in (False, True):
        for N, M in ((5, 257), (1025, 1025)):
            R = _set(ahv, N, per_sample).to(dev)
            keys, _ = _keys(ahv, N, dev)
            for sigma, max_angle in ((3.0, None), (30.0, None), (3.0, 2.0)):
                kw = dict(idx=_idx(N, M).to(dev), sigma_deg=sigma, step=_step(dev), seed=SEED, best_key=keys, n_fresh=16,
                          max_angle_deg=max_angle, want_omega=True)
                a, wa = ops.diffuse_rotations(R, **kw)
                b, vel, wb = ops.predict_rotations(R, None, sigma_vel_deg=0.0, damping=1.0, coast=False, **kw)
                assert not vel.any()
                worst = max(worst, float((a.double() - b.double()).abs().max()))
                worst_w = max(worst_w, float((wa.double() - wb.double()).abs().max()))
    print("predict_rotations without velocities against diffuse_rotations: max |entry| difference %.3e, of omega %.3e (bar %.3e)"
          % (worst, worst_w, bar))
    assert worst <= bar and worst_w <= bar


# ---- 4. noise ------------------------------------------------------------------------------------------------------------
def test_noise_is_standard_normal_and_independent(ahv, ops, dev):
    M, sigma, sigma_vel = 12288, 3.0, 1.0
    R = _set(ahv, 5, True).to(dev)          # per sample: B comes from R
    out, vel, om = ops.predict_rotations(R, m=M, sigma_deg=sigma, sigma_vel_deg=sigma_vel, step=_step(dev), seed=SEED,
                                         want_omega=True)
    vel, om = vel.cpu().double().numpy().reshape(-1, 3), om.cpu().double().numpy().reshape(-1, 3)
    z = np.concatenate([(om - vel) / f32(math.radians(sigma)), vel / f32(math.radians(sigma_vel))], axis=1)   # (n, 6)
    n = z.shape[0]
    assert n == B * M == 36864
    band, five = dkw(n), 5.0 / math.sqrt(n)
    gaps = [ecdf_gap(z[:, c], PHI) for c in range(6)]
    corr = np.abs(np.corrcoef(z.T) - np.eye(6))
    print("noise (omega_p / sigma, velocity noise / sigma_vel), n = %d: ECDF gaps %s (band %.4f); means %s, deviations %s, largest "
          "correlation %.4f (bound %.4f)" % (n, ["%.4f" % x for x in gaps], band, ["%.4f" % x for x in z.mean(0)],
                                             ["%.4f" % x for x in z.std(0)], corr.max(), five))
    for c in range(6):
        assert gaps[c] <= band
        assert abs(z[:, c].mean()) <= five
        assert abs(z[:, c].std() - 1.0) <= 5.0 / math.sqrt(2 * n)      # a sample deviation's standard error is 1 / sqrt(2 n)
    assert corr.max() <= five


def test_velocity_noise_of_a_slot_depends_on_seed_step_b_j_only(ahv, ops, dev):
    N = 1025
    R, V = _set(ahv, N, True).to(dev), _vel(N, True).to(dev)
    g = torch.Generator().manual_seed(1)

    def call(M, idx=None, V=None, seed=SEED, t=STEP):    # damping 0: vel_out is the slot's velocity noise itself
        return ops.predict_rotations(R, V, idx=idx, m=None if idx is not None else M, sigma_deg=3.0, sigma_vel_deg=1.0, damping=0.0,
                                     step=_step(dev, t), seed=seed)[1]

    base = call(1025)
    assert base.abs().sum(-1).min() > 0
    assert torch.equal(call(100), base[:, :100])
    for _ in range(2):
        idx = torch.randint(0, N, (B, 1025), generator=g, dtype=torch.int64).to(dev)
        assert torch.equal(call(1025, idx)[:, :100], base[:, :100])
        assert torch.equal(call(1025, idx, V), base)
    assert not torch.equal(call(100, seed=SEED + 1), base[:, :100])
    assert not torch.equal(call(100, t=STEP + 1), base[:, :100])
    assert not torch.equal(base[0], base[1])


# ---- 5. limits -------------------------------------------------------------------------------------------------------------
def test_max_speed_clips_the_velocity(ahv, ops, dev):
    N, M, max_deg = 1025, 1025, 5.0
    R, V = _set(ahv, N, False).to(dev), _vel(N, False, deg=10.0)
    idx = _idx(N, M, seed=2)
    bound = f32(math.radians(max_deg))                                      # what the entry point is given
    assert (np.linalg.norm(cv.gather_vel(V.double().numpy(), idx.numpy()), axis=-1) > bound).mean() > 0.9      # rows feeding in |v| > 5 deg
    kw = dict(idx=idx.to(dev), sigma_deg=3.0, sigma_vel_deg=30.0, damping=1.0, step=_step(dev), seed=SEED, want_omega=True)
    _, free, om0 = (x.cpu() for x in ops.predict_rotations(R, V.to(dev), **kw))
    _, vel, om = (x.cpu() for x in ops.predict_rotations(R, V.to(dev), max_speed_deg=max_deg, **kw))
    was, norm = np.linalg.norm(free.double().numpy(), axis=-1), np.linalg.norm(vel.double().numpy(), axis=-1)
    print("max_speed %.1f deg: %.1f%% of the slots clipped, largest |v| / bound = %.9f" % (max_deg, 100 * (was > bound).mean(),
                                                                                          norm.max() / bound))
    assert (was > bound).mean() > 0.5                                       # the reference: the limit bites on most slots
    assert norm.max() <= bound
    assert norm[was > bound].min() >= bound * (1 - 1e-5)                    # clipped to the limit, not below it
    # a velocity inside the limit is untouched: slower rows and sigma_vel = 1 degree, where about half the slots stay inside
    slow = dict(kw, sigma_vel_deg=1.0)
    _, free1, _ = ops.predict_rotations(R, _vel(N, False, deg=3.0).to(dev), **slow)
    _, vel1, _ = ops.predict_rotations(R, _vel(N, False, deg=3.0).to(dev), max_speed_deg=max_deg, **slow)
    was1 = np.linalg.norm(free1.cpu().double().numpy(), axis=-1)
    inside = was1 < bound * (1 - 1e-5)
    assert 0.2 < inside.mean() < 0.8 and np.linalg.norm(vel1.cpu().double().numpy(), axis=-1).max() <= bound
    assert torch.equal(vel1.cpu()[_t(inside)], free1.cpu()[_t(inside)])
    # the pose noise is not touched by max_speed: omega - v' is the same vector in both runs, up to the rounding of the two
    # sums (half an ulp each of components below 4 rad: 2^-23 together)
    assert float(om0.abs().max()) < 4.0
    assert float(((om.double() - vel.double()) - (om0.double() - free.double())).abs().max()) <= 2.0 ** -23


def test_max_angle_behaves_as_in_diffuse(ahv, ops, dev, accuracy):
    N, M, max_deg = 1025, 1025, 2.0
    R = _set(ahv, N, False).to(dev)
    kw = dict(idx=_idx(N, M, seed=2).to(dev), sigma_deg=3.0, step=_step(dev), seed=SEED, max_angle_deg=max_deg, want_omega=True)
    _, wd = ops.diffuse_rotations(R, **kw)
    _, _, wp = ops.predict_rotations(R, None, sigma_vel_deg=0.0, **kw)
    bound = f32(math.radians(max_deg))
    norm = np.linalg.norm(wp.cpu().double().numpy(), axis=-1)
    assert norm.max() <= bound and (norm >= bound * (1 - 1e-5)).mean() > 0.5
    assert float((wd.double() - wp.double()).abs().max()) <= 4.0 * accuracy[1]
    # with velocities the limit holds for the noise term alone: omega - v' (rounded once more by the sum)
    V = _vel(N, False).to(dev)
    _, vel, om = ops.predict_rotations(R, V, sigma_vel_deg=1.0, **kw)
    part = np.linalg.norm((om.cpu().double() - vel.cpu().double()).numpy(), axis=-1)
    assert part.max() <= bound + 3 * 2.0 ** -24 * float(om.abs().max())


# ---- 6. a bad row stays with its slots -------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True])
def test_bad_rows_change_no_other_slot(ahv, ops, dev, per_sample):
    N, M, F = 5, 257, 16
    R, V = _set(ahv, N, per_sample), _vel(N, per_sample)
    idx = _idx(N, M, seed=4)
    best = np.array([0, 2, 4], np.int64)
    keys = _t(ahv.dist.pack_keys_host(np.full(B, 0.5, np.float32), best)).to(dev)
    run = lambda X, Y: [x.cpu() for x in ops.predict_rotations(X.to(dev), Y.to(dev), idx=idx.to(dev), sigma_deg=3.0, step=_step(dev),
                                                               seed=SEED, best_key=keys, n_fresh=F, want_omega=True)]
    for what in ("R", "V"):
        bad_R, bad_V = R.clone(), V.clone()
        if what == "R":
            bad_R[..., 2, :, :] = 0.0
            bad_R[..., 3, :, :] = float("nan")
            rows = (2, 3)
        else:
            bad_V[..., 1, :] = float("nan")
            bad_V[..., 2, :] = 0.0
            rows = (1, 2)
        src = idx.clone()
        src[:, 0] = src[:, 1] = _t(best)                  # the elite and the coast slot read the key's row
        reads_bad = (src == rows[0]) | (src == rows[1])
        reads_bad[:, M - F:] = False                      # fresh slots read nothing
        assert reads_bad[:, 2:].any() and reads_bad[:, :2].any() and not reads_bad[:, :2].all()
        clean = ~reads_bad
        a, b = run(R, V), run(bad_R, bad_V)
        for x, y in zip(a, b):
            assert _bytes_equal(x[clean], y[clean]), what
        assert not _bytes_equal(a[0][reads_bad], b[0][reads_bad]), what      # (the bad rows did reach their own slots)


# ---- 6b. the op's host checks on device tensors ------------------------------------------------------------------------------
def test_op_refuses_bad_device_arguments(ahv, ops, dev):
    N, M = 5, 7
    R, V = _set(ahv, N, True).to(dev), _vel(N, True).to(dev)
    idx = torch.zeros((B, M), dtype=torch.int64, device=dev)
    step = _step(dev)
    call = lambda **kw: ops.predict_rotations(R, **dict(dict(V=V, idx=idx, sigma_deg=3.0, step=step, seed=SEED), **kw))
    assert len(call()) == 2 and len(call(want_omega=True)) == 3                # the base call is accepted
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    for kw, word in ((dict(m=M + 1), "disagrees with idx"), (dict(idx=idx.int()), "int64"), (dict(idx=idx.cpu()), "same device"),
                     (dict(n_fresh=M + 1), "n_fresh"), (dict(V=V[:, :4]), "V must be"), (dict(V=V[:2]), "V must be"),
                     (dict(V=e(B, N, 4)), "V must be"), (dict(V=V.double()), "float32"), (dict(V=V.cpu()), "no CPU fallback"),
                     (dict(best_key=torch.zeros(B + 1, dtype=torch.int64, device=dev)), "best_key"),
                     (dict(out=e(B, M + 1, 3, 3)), "out must be"), (dict(vel_out=e(B, M, 4)), "vel_out must be"),
                     (dict(vel_out=e(B, M, 3).double()), "vel_out must be"), (dict(omega_out=e(B, M + 1, 3)), "omega_out must be"),
                     (dict(step=None), "step is required"), (dict(step=step.cpu()), "no CPU fallback"),
                     (dict(sigma_deg=float("inf")), "sigma_deg"), (dict(sigma_vel_deg=-1.0), "sigma_vel_deg"),
                     (dict(damping=1.5), "damping"), (dict(damping=float("nan")), "damping"),
                     (dict(max_angle_deg=-1.0), "max_angle_deg"), (dict(max_speed_deg=float("nan")), "max_speed_deg")):
        with pytest.raises(RuntimeError, match=word):
            call(**kw)
    # out inside R's memory, vel_out inside V's
    big = e(B * N * 9 + B * M * 9)
    Rv = big[:B * N * 9].view(B, N, 3, 3).copy_(R)
    with pytest.raises(RuntimeError, match="out must not overlap R"):
        ops.predict_rotations(Rv, V, idx=idx, step=step, out=big[9:9 + B * M * 9].view(B, M, 3, 3))
    bigv = e(B * N * 3 + B * M * 3)
    Vv = bigv[:B * N * 3].view(B, N, 3).copy_(V)
    for off in (0, 3, B * N * 3 - 1):
        with pytest.raises(RuntimeError, match="vel_out must not overlap V"):
            ops.predict_rotations(R, Vv, idx=idx, step=step, vel_out=bigv[off:off + B * M * 3].view(B, M, 3))
    out, vel, om = big[B * N * 9:].view(B, M, 3, 3), bigv[B * N * 3:].view(B, M, 3), e(B, M, 3)      # right behind: accepted
    got = ops.predict_rotations(Rv, Vv, idx=idx, sigma_deg=3.0, step=step, seed=SEED, out=out, vel_out=vel, omega_out=om)
    assert got[0] is out and got[1] is vel and got[2] is om
    want = call(want_omega=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


# ---- 7. PoseTracker ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(dev):
    g, h = load_golden("batched"), load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    return _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev), w


def _frames(vt, n):
    """n target volumes from the fixture's: its samples rolled and blended, so that every frame differs."""
    return [(0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous() for k in range(n)]


def _tracker(ahv, w, seed=1, **kw):
    a = dict(particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=seed, motion="constant_velocity",
             sigma_vel_deg=1.0, damping=0.9)
    a.update(kw)
    return ahv.track.PoseTracker(*w, **a)


NAMES = ("particles", "scores", "score", "idx", "R_map", "reacquired")


def _trajectory(ahv, dev, pair, steps=4, **kw):
    """[(TrackStep, velocities)] of init and ``steps`` steps, cloned."""
    vs, vt, w = pair
    t = _tracker(ahv, w, **kw)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    outs = [(t.init(vs, vt, R0), None)]
    for f in _frames(vt, steps):
        o = t.step(vs, f)
        outs.append((type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o]), t.velocities.clone()))
    return outs


def test_same_seed_same_bytes(ahv, ops, dev, pair):
    a, b, c = (_trajectory(ahv, dev, pair, seed=s) for s in (1, 1, 2))
    for (x, vx), (y, vy) in zip(a[1:], b[1:]):
        for name in NAMES + ("draws",):
            assert torch.equal(getattr(x, name), getattr(y, name)), name
        assert _bytes_equal(vx, vy)
    assert not torch.equal(a[1][0].particles, c[1][0].particles) and not torch.equal(a[1][1], c[1][1])
    # the step is the op's: slot 0 the previous arg-max, slot 1 that pose moved by its velocity, reacquired behind both
    for (prev, vprev), (cur, vcur) in zip(a[1:], a[2:]):
        rows = torch.arange(B, device=dev)
        assert torch.equal(cur.particles[:, 0], prev.R_map)
        assert torch.equal(vcur[:, 0], vprev[rows, prev.idx]) and torch.equal(vcur[:, 1], vprev[rows, prev.idx])
        assert torch.equal(cur.reacquired, cur.idx >= 257 - 8)
    assert a[1][1][:, :2].abs().max() == 0          # the first step after init starts from zero velocities


def test_captured_steps_equal_eager_steps(ahv, ops, dev, pair):
    steps = 6
    eager = _trajectory(ahv, dev, pair, steps=steps)
    graphed = _trajectory(ahv, dev, pair, steps=steps, use_graph=True)
    for k, ((x, vx), (y, vy)) in enumerate(zip(eager, graphed)):
        for name in NAMES:
            assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (k, name)
        if k:
            assert torch.equal(x.draws, y.draws), k
            assert _bytes_equal(vx, vy), k


def test_chained_prediction_stays_on_so3_and_bounded(ahv, ops, dev):
    M, max_deg = 257, 5.0
    defect = lambda R: float((R.double().transpose(-1, -2) @ R.double() - torch.eye(3, dtype=torch.float64)).abs().max())
    fresh = ops.random_rotations(B * M, seed=3, device=dev).reshape(B, M, 3, 3)
    bufs, vels = [fresh.clone(), torch.empty_like(fresh)], [torch.zeros((B, M, 3), device=dev) for _ in range(2)]
    step = _step(dev, 0)
    bound, largest = f32(math.radians(max_deg)), 0.0
    for k in range(256):
        p = k & 1
        ops.predict_rotations(bufs[p], vels[p] if k else None, sigma_deg=3.0, sigma_vel_deg=1.0, damping=1.0, step=step, seed=SEED,
                              max_speed_deg=max_deg, out=bufs[1 - p], vel_out=vels[1 - p])
        step += 1
        if k % 32 == 31:
            largest = max(largest, float(np.linalg.norm(vels[1 - p].cpu().double().numpy(), axis=-1).max()))
    got, base = defect(bufs[0].cpu()), defect(fresh.cpu())
    print("max |R^T R - I| after 256 chained calls %.3e; random_rotations output of the same size %.3e; largest |v| / bound %.6f"
          % (got, base, largest / bound))
    assert got <= 4.0 * base
    assert 0.5 * bound < largest <= bound           # the velocities did random-walk into the limit, and stayed inside it
    assert float(tr.geodesic_deg(fresh.cpu().numpy(), bufs[0].cpu().numpy()).min()) > 1.0      # (the particles did move)


def test_tracker_velocities_stay_bounded(ahv, ops, dev, pair):
    vs, vt, w = pair
    max_deg = 2.0
    t = _tracker(ahv, w, damping=1.0, sigma_vel_deg=2.0, max_speed_deg=max_deg)
    t.init(vs, vt, _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev))
    bound, seen = f32(math.radians(max_deg)), 0.0
    for f in _frames(vt, 8) * 4:
        out = t.step(vs, f)
        assert tuple(t.velocities.shape) == (B, 257, 3)
        seen = max(seen, float(np.linalg.norm(t.velocities.cpu().double().numpy(), axis=-1).max()))
    assert 0.5 * bound < seen <= bound


# ---- 8. the fast planted sequence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_fast_planted_sequence_on_the_device(ahv, ops, dev, s):
    P = cv.FAST
    h = load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    vs = _t(h["vol_src"]).to(dev)
    R0 = _t(tr.planted_init(ahv.rotations, s)).to(dev)
    trackers = {}
    for motion in ("walk", "constant_velocity"):
        t = ahv.track.PoseTracker(*w, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                  temperature=P["temperature"], batch=1, seed=s, motion=motion, sigma_vel_deg=P["sigma_vel_deg"],
                                  damping=P["damping"])
        trackers[motion] = (lambda vt, t=t: t.init(vs, vt, R0), lambda vt, t=t: t.step(vs, vt))
    rotate = lambda R: ops.rotate_volume(vs, _t(R[None].astype(np.float32)).to(dev))
    err = cv.run(ahv.rotations, s, P, rotate, trackers)
    worst, median = cv.fast_bar(err["constant_velocity"], err["walk"])
    for name in ("walk", "constant_velocity"):
        print("fast planted s=%d on the device, %-17s: %s" % (s, name, " ".join("%.2f" % e for e in err[name])))
    print("fast planted s=%d on the device: constant-velocity late max %.3f | walk late median %.3f" % (s, worst, median))
    assert worst < median
