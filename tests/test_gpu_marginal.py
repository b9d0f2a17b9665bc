"""Marginal smoothing on the device: ``ahv_marginal_step_f32`` / ``ahv_marginal_smooth_f32`` against the fp64 reference
(tests/marginal_reference.py) and ``track.PoseTracker(history=H, marginals=True)``.

Shapes: B = 3, M in {1, 5, 16, 17, 255, 257, 1025} -- a lone row, a partial owner block, exactly one owner block and one row
more, a partial tile (255), one row into the second tile (257) and several tiles with the register prefetch -- and H in
{2, 3, 5} with more steps than H.

The bar of every accuracy check is the project's: 4 x the error of the stock fp32 torch composition (the M x M x 9 differences,
``torch.logsumexp``, on the CPU) against the same fp64 numbers, both computed here from the SAME stored fp32 inputs (the
device's own ring), over the entries that are finite in the reference.  This file prints every figure before it asserts.

Figures measured on the MI355X (DESIGN 4.2 quotes them), kernel / stock, largest over all M:
  alpha against fp64: 3.9e-06 / 3.9e-06 at sigma 3 deg, 3.9e-06 / 3.8e-06 at 30 deg, 3.8e-06 / 3.9e-06 and 3.9e-06 / 3.9e-06 with
  velocities; log gamma (F = 3): 8.3e-06 / 1.0e-05, 8.1e-06 / 8.8e-06, 7.7e-06 / 1.0e-05 and 7.8e-06 / 1.1e-05; |sum exp - 1| 2.0e-06
  far clusters (jump +inf, w about -365): alpha 7.2e-05 / 7.2e-05, log gamma 1.2e-04 / 1.9e-04, every value finite
  planted distractor, max over frames 4-11 of the marginal arg-max / the posterior mean pose / the blind median, degrees:
  3.81 / 3.70 / 8.44; 4.13 / 4.12 / 8.00; 2.84 / 2.91 / 7.01
"""
import math

import numpy as np
import pytest
import torch

from . import marginal_reference as mg
from . import smooth_reference as sm
from . import track_reference as tr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
B = 3
MS, HS = (1, 5, 16, 17, 255, 257, 1025), (2, 3, 5)
INF = float("inf")
T = 0.02


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


def _step(dev, value):
    return torch.full((1,), value, dtype=torch.int64, device=dev)


def _bytes_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


PATTERN = 0x7FC00000


def _nan_rings(ops, dev, nb, M, H, velocities=False):
    """Rings whose every word is the NaN pattern 0x7FC00000."""
    h, m = ops.smooth_history(nb, M, H, dev, velocities=velocities), ops.marginal_history(nb, M, H, dev)
    for x in tuple(h) + tuple(m):
        if x is not None:
            x.view(torch.int32).fill_(PATTERN)
    return h, m


def _cloud(ahv, M, sigma_deg, seed, frames, nb=B):
    """frames sets (nb,M,3,3) fp32: a Haar pose per sample, every particle diffused by sigma; scores (nb,M) in [-1, 1]."""
    rs = np.random.RandomState(seed)
    base = ahv.rotations.haar_rotations_np(nb, seed=seed).astype(np.float64)
    Rs = [(base[:, None] @ tr.exp_so3(math.radians(sigma_deg) * rs.standard_normal((nb, M, 3)))).astype(np.float32) for _ in range(frames)]
    scores = [rs.uniform(-1, 1, (nb, M)).astype(np.float32) for _ in range(frames)]
    return Rs, scores


def _chain(ops, dev, H, Rs, scores, sigma_deg, jump, Vs=None, first_step=1, rings=None, temperature=T, each=None):
    """smooth_step (records the frame) and marginal_step per frame, the marginal step first on even frames; ``each(f, t, hist,
    marg)`` after every frame."""
    nb, M = scores[0].shape
    hist, marg = _nan_rings(ops, dev, nb, M, H, velocities=Vs is not None) if rings is None else rings
    for f, (R, s) in enumerate(zip(Rs, scores)):
        t = first_step + f
        Rd, sd, st = _t(R).to(dev), _t(s).to(dev), _step(dev, t)
        rec = lambda: ops.smooth_step(hist, Rd, sd, st, temperature, sigma_deg, jump=jump, V=_t(Vs[f]).to(dev) if Vs is not None else None,
                                      damping=0.9, first_step=first_step)
        if f % 2:
            rec()
        ops.marginal_step(hist, marg, Rd, sd, st, temperature, sigma_deg, jump=jump, first_step=first_step)
        if not f % 2:
            rec()
        if each is not None:
            each(f, t, hist, marg)
    return hist, marg


# ---- the fp64 reference and the stock fp32 composition on the device's own stored inputs --------------------------------------
def _host_rings(hist, marg):
    """(MarginalRing fp64 of the device's stored fp32 rings, the fp32 host tensors)."""
    H, nb, M = hist.R.shape[:3]
    ring = sm.Ring(H, nb, M, velocities=hist.P is not None)
    ring.R = hist.R.cpu().double().numpy()
    if hist.P is not None:
        ring.P = hist.P.cpu().double().numpy()
    mr = mg.MarginalRing(ring)
    mr.alpha, mr.emit = marg.alpha.cpu().double().numpy(), marg.emit.cpu().double().numpy()
    return mr


def _stock_w(P, R, k, jump):
    """(Mi, Mj) fp32: the transition from the M x M x 9 differences."""
    diff = P.reshape(-1, 1, 9) - R.reshape(1, -1, 9)
    return torch.clamp(-(diff * diff).sum(-1) * float(np.float32(k)), min=-jump)


def _stock_forward(R, s, P_prev, a_prev, beta, k, jump):
    m = a_prev[torch.isfinite(a_prev)].max()
    return float(np.float32(beta)) * s + torch.logsumexp((a_prev - m)[:, None] + _stock_w(P_prev, R, k, jump), dim=0)


def _stock_smooth(mr32, t, F, k, jump):
    """The stock fp32 backward recursion and finish for one sample: mr32 = (R, P, alpha, emit) fp32 (H,M,...) of that sample."""
    R, P, alpha, emit = mr32
    H = R.shape[0]
    out = []
    beta = torch.zeros_like(alpha[0])
    for back in range(F):
        slot = (t - back) % H
        out.append(torch.log_softmax(alpha[slot] + beta, dim=0))
        if back + 1 < F:
            g = emit[slot] + beta
            beta = torch.logsumexp(_stock_w(P[(t - back - 1) % H], R[slot], k, jump) + (g - g[torch.isfinite(g)].max())[None, :], dim=1)
    return torch.stack(out[::-1])


def _err(got, want):
    """Largest |got - want| over the entries finite in ``want``; the non-finite ones must agree exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return float(np.abs(got[fin] - want[fin]).max(initial=0.0))


def _forward_errors(ops, hist, marg, t, R, s, sigma_deg, jump, first_step=1):
    """(kernel error, stock error) of alpha of frame t against fp64, from the device's stored previous slot; emit and the
    finite pattern are checked exactly."""
    H, nb, M = hist.R.shape[:3]
    mr = _host_rings(hist, marg)
    beta, k = ops.inverse_temperature(T), sm.inv4s2(ops._angle_rad(sigma_deg, "sigma_deg"))
    slot, prev = t % H, (t - 1) % H
    Pp = mr.ring.P if mr.ring.P is not None else mr.ring.R
    kern = stock = 0.0
    for b in range(nb):
        want_a, want_e = mg.forward_step(R[b], s[b], beta, k, jump, Pp[prev, b], mr.alpha[prev, b]) if t > first_step else \
            mg.forward_step(R[b], s[b], beta, k, jump)
        assert np.array_equal(np.isfinite(mr.alpha[slot, b]), np.isfinite(want_a)), (M, t, b)
        assert _bytes_equal(marg.emit[slot, b], _t(want_e.astype(np.float32))), (M, t, b)
        kern = max(kern, _err(mr.alpha[slot, b], want_a))
        if t > first_step:
            st = _stock_forward(_t(R[b]), _t(s[b]), _t(Pp[prev, b].astype(np.float32)), _t(mr.alpha[prev, b].astype(np.float32)), beta, k, jump)
            stock = max(stock, _err(st.double().numpy(), want_a))
        else:
            assert _bytes_equal(marg.alpha[slot, b], marg.emit[slot, b])
    return kern, stock


def _smooth_errors(ops, dev, hist, marg, t, F, sigma_deg, jump, first_step=1, check_idx=True, stock_samples=None):
    """(kernel error, stock error, largest |sum exp(log gamma) - 1|, the SmoothedMarginals) of the newest F frames against fp64.
    ``stock_samples``: the samples the stock composition runs on (it has no notion of a dead particle); default all."""
    H, nb, M = hist.R.shape[:3]
    res = ops.marginal_smooth(hist, marg, _step(dev, t), sigma_deg, jump=jump, frames=F, first_step=first_step)
    mr = _host_rings(hist, marg)
    sigma = ops._angle_rad(sigma_deg, "sigma_deg")
    want, want_idx, want_R = mr.smooth(t, F, sigma, jump, first_step)
    got = res.logw.cpu().double().numpy()
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.all(got[~np.isfinite(want)] == -np.inf)
    kern, stock, total = _err(got, want), 0.0, 0.0
    Fr = min(F, t - first_step + 1)                      # the recorded ones
    P32 = (hist.P if hist.P is not None else hist.R).cpu()
    for b in (range(nb) if stock_samples is None else stock_samples):
        st = _stock_smooth((hist.R[:, b].cpu(), P32[:, b], marg.alpha[:, b].cpu(), marg.emit[:, b].cpu()), t, Fr, sm.inv4s2(sigma), jump)
        stock = max(stock, _err(st.double().numpy(), want[b, F - Fr:]))
    alive = np.isfinite(want).any(axis=-1)
    if alive.any():
        total = float(np.abs(np.exp(got).sum(axis=-1) - 1.0)[alive].max())
    if check_idx:
        idx = res.idx.cpu().numpy()
        top = np.sort(np.where(np.isfinite(want), want, -np.inf), axis=-1)
        with np.errstate(invalid="ignore"):               # (-inf - -inf in a frame without a live particle: not ``alive``)
            gap = top[..., -1] - top[..., -2] if M > 1 else np.full(want.shape[:2], np.inf)
        clear = alive & (gap > 4.0 * stock)
        assert np.array_equal(idx[clear], want_idx[clear]) and np.all(idx[~alive] == -1) and np.all(idx[alive] >= 0)
        # the pose is the ring's row, bit for bit; the identity for -1
        Rg = res.R.cpu()
        for b in range(nb):
            for f in range(F):
                row = torch.eye(3) if idx[b, f] < 0 else hist.R[(t - (F - 1 - f)) % H, b, int(idx[b, f])].cpu()
                assert _bytes_equal(Rg[b, f], row), (b, f)
        # the stored index is the FIRST arg-max of the stored row
        assert np.array_equal(idx[alive], np.argmax(res.logw.cpu().numpy(), axis=-1)[alive])
    return kern, stock, total, res


# ---- 1. accuracy on random clouds -----------------------------------------------------------------------------------------
_ACC = {}


def _accuracy(ahv, ops, dev, sigma_deg, vel):
    """Pooled over every M: H = 3, four frames (the ring wraps), jump 8.  alpha of the last frame and log gamma of the newest
    three frames, kernel and stock against fp64."""
    key = (sigma_deg, vel)
    if key not in _ACC:
        fk = fs = sk = ss = tot = 0.0
        for M in MS:
            Rs, scores = _cloud(ahv, M, sigma_deg, 7 * M + int(sigma_deg), 4)
            rs = np.random.RandomState(M)
            Vs = [(math.radians(sigma_deg) * rs.standard_normal((B, M, 3))).astype(np.float32) for _ in range(4)] if vel else None
            hist, marg = _chain(ops, dev, 3, Rs, scores, sigma_deg, 8.0, Vs=Vs)
            a, b = _forward_errors(ops, hist, marg, 4, Rs[3], scores[3], sigma_deg, 8.0)
            c, d, e, _ = _smooth_errors(ops, dev, hist, marg, 4, 3, sigma_deg, 8.0)
            print("M %4d sigma %4.1f vel %d: alpha kernel %.3e stock %.3e | log gamma kernel %.3e stock %.3e | sum-1 %.3e"
                  % (M, sigma_deg, vel, a, b, c, d, e))
            fk, fs, sk, ss, tot = max(fk, a), max(fs, b), max(sk, c), max(ss, d), max(tot, e)
        _ACC[key] = (fk, fs, sk, ss, tot)
    return _ACC[key]


CONFIGS = [(3.0, False), (3.0, True), (30.0, False), (30.0, True)]


@pytest.mark.parametrize("sigma_deg,vel", CONFIGS)
def test_alpha_matches_fp64(ahv, ops, dev, sigma_deg, vel):
    fk, fs, _, _, _ = _accuracy(ahv, ops, dev, sigma_deg, vel)
    print("alpha sigma %4.1f deg, velocities %d: max |alpha - fp64| kernel %.3e, stock fp32 torch %.3e" % (sigma_deg, vel, fk, fs))
    assert fk <= 4.0 * fs


@pytest.mark.parametrize("sigma_deg,vel", CONFIGS)
def test_log_gamma_matches_fp64_and_sums_to_one(ahv, ops, dev, sigma_deg, vel):
    _, _, sk, ss, tot = _accuracy(ahv, ops, dev, sigma_deg, vel)
    print("log gamma sigma %4.1f deg, velocities %d: max |log gamma - fp64| kernel %.3e, stock fp32 torch %.3e; max |sum exp - 1| %.3e"
          % (sigma_deg, vel, sk, ss, tot))
    assert sk <= 4.0 * ss
    assert tot <= 4.0 * ss


# ---- 2. the ring: wraps, first_step, frames never recorded -------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
def test_ring_wraps_and_first_step(ahv, ops, dev, H):
    first = (1 << 33) + 4                                          # int64 slot arithmetic: 2^33 + 4 is not 4
    for M in (17, 257):
        frames = H + 2
        Rs, scores = _cloud(ahv, M, 3.0, 31 * M + H, frames)
        pattern = torch.full((B, M), PATTERN, dtype=torch.int32)
        fk = fs = sk = ss = tot = 0.0

        def each(f, t, hist, marg):
            nonlocal fk, fs, sk, ss, tot
            a, b = _forward_errors(ops, hist, marg, t, Rs[f], scores[f], 3.0, 8.0, first_step=first)
            fk, fs = max(fk, a), max(fs, b)
            if f == 0:                                             # only the frame's own slot has been written
                for k in range(H):
                    if k != t % H:
                        assert torch.equal(marg.alpha[k].view(torch.int32).cpu(), pattern)
                        assert torch.equal(marg.emit[k].view(torch.int32).cpu(), pattern)
            if f % 2 == 0 or f == frames - 1:
                c, d, e, res = _smooth_errors(ops, dev, hist, marg, t, H, 3.0, 8.0, first_step=first)
                sk, ss, tot = max(sk, c), max(ss, d), max(tot, e)
                n_rec = min(H, f + 1)
                assert (res.idx[:, :H - n_rec] == -1).all() and (res.idx[:, H - n_rec:] >= 0).all()
                assert (res.logw[:, :H - n_rec] == -INF).all()
                for k in range(H - n_rec):
                    assert _bytes_equal(res.R[:, k], torch.eye(3).expand(B, 3, 3))

        hist, marg = _chain(ops, dev, H, Rs, scores, 3.0, 8.0, first_step=first, each=each)
        print("H %d M %d: alpha kernel %.3e stock %.3e | log gamma kernel %.3e stock %.3e | sum-1 %.3e" % (H, M, fk, fs, sk, ss, tot))
        assert fk <= 4.0 * fs and sk <= 4.0 * ss and tot <= 4.0 * ss
        # a shorter window and ``out``
        t = first + frames - 1
        out = ops.SmoothedMarginals(torch.empty((B, 1, M), device=dev), torch.empty((B, 1), dtype=torch.int64, device=dev),
                                    torch.empty((B, 1, 3, 3), device=dev))
        got = ops.marginal_smooth(hist, marg, _step(dev, t), 3.0, frames=1, first_step=first, out=out)
        assert got.logw.data_ptr() == out.logw.data_ptr() and got.idx.data_ptr() == out.idx.data_ptr()
        want = torch.log_softmax(marg.alpha[t % H].cpu().double(), dim=-1)
        assert float((out.logw[:, 0].cpu().double() - want).abs().max()) < 1e-5
        # a step with the same counter but first_step = t has no predecessors, whatever the ring holds
        ops.marginal_step(hist, marg, _t(Rs[-1]).to(dev), _t(scores[-1]).to(dev), _step(dev, t), T, 3.0, first_step=t)
        assert _bytes_equal(marg.alpha[t % H], marg.emit[t % H])
        assert _bytes_equal(marg.emit[t % H], _t((np.float32(ops.inverse_temperature(T)) * scores[-1]).astype(np.float32)))


# ---- 3. no underflow ------------------------------------------------------------------------------------------------------------
def test_far_clusters_do_not_underflow(ahv, ops, dev):
    """jump = +inf, sigma 3 degrees, the predecessors within half a degree of one pose and the successors 90 degrees away: every
    transition is about -365 nats, exp of which is 0 in fp32.  A running maximum keeps every particle alive."""
    for M in (17, 257):
        rs = np.random.RandomState(M)
        base = ahv.rotations.haar_rotations_np(B, seed=3).astype(np.float64)
        quarter = tr.exp_so3(np.array([0.0, 0.0, math.pi / 2]))
        near = lambda c: (c[:, None] @ tr.exp_so3(math.radians(0.5) * rs.standard_normal((B, M, 3)))).astype(np.float32)
        Rs = [near(base), near(base @ quarter), near(base)]
        scores = [rs.uniform(-1, 1, (B, M)).astype(np.float32) for _ in range(3)]
        hist, marg = _chain(ops, dev, 3, Rs, scores, 3.0, INF)
        mr = _host_rings(hist, marg)
        w = sm.transition(mr.ring.R[1, 0], Rs[1][0], sm.inv4s2(math.radians(3.0)), INF)
        assert w.max() < -300.0                                                    # the premise: exp(-104) is already 0 in fp32
        assert torch.isfinite(marg.alpha).all()
        a, b = _forward_errors(ops, hist, marg, 2, Rs[1], scores[1], 3.0, INF)
        c, d, e, res = _smooth_errors(ops, dev, hist, marg, 3, 3, 3.0, INF)
        print("far clusters M %d: alpha kernel %.3e stock %.3e | log gamma kernel %.3e stock %.3e | sum-1 %.3e" % (M, a, b, c, d, e))
        assert torch.isfinite(res.logw).all() and (res.idx >= 0).all()
        assert a <= 4.0 * b and c <= 4.0 * d and e <= 4.0 * d


# ---- 4. isolation and the -inf / -1 / identity rules -------------------------------------------------------------------------------
def test_bad_values_stay_with_their_sample(ahv, ops, dev):
    """Five frames, H = 5.  Sample 1 is the bad one: a NaN pose in frame 2, a NaN, a +inf and a -inf score in frame 3, every
    score of frame 4 non-finite.  Samples 0 and 2 keep the bytes of the clean run, and sample 1 follows the reference's rules."""
    M, H, frames = 257, 5, 5
    Rs, scores = _cloud(ahv, M, 3.0, 77, frames)
    clean_h, clean_m = _chain(ops, dev, H, Rs, scores, 3.0, 8.0)
    clean = ops.marginal_smooth(clean_h, clean_m, _step(dev, frames), 3.0)
    Rs, scores = [R.copy() for R in Rs], [s.copy() for s in scores]
    Rs[1][1, 7] = np.nan
    scores[2][1, 5], scores[2][1, 100], scores[2][1, 256] = np.nan, np.inf, -np.inf
    scores[3][1, :] = np.nan
    scores[3][1, ::2] = np.inf
    hist, marg = _chain(ops, dev, H, Rs, scores, 3.0, 8.0)
    c, d, e, res = _smooth_errors(ops, dev, hist, marg, frames, H, 3.0, 8.0, stock_samples=(0, 2))
    print("bad values: log gamma kernel (all samples) %.3e stock (samples 0 and 2) %.3e | sum-1 %.3e" % (c, d, e))
    assert c <= 4.0 * d and e <= 4.0 * d
    for b in (0, 2):
        assert _bytes_equal(marg.alpha[:, b], clean_m.alpha[:, b]) and _bytes_equal(marg.emit[:, b], clean_m.emit[:, b])
        assert _bytes_equal(res.logw[b], clean.logw[b]) and torch.equal(res.idx[b], clean.idx[b]) and _bytes_equal(res.R[b], clean.R[b])
    a, em, lw, idx = marg.alpha.cpu(), marg.emit.cpu(), res.logw.cpu(), res.idx.cpu()
    # frame 2 (slot 2): the NaN pose is alive (its score is finite) but no edge reaches it
    assert a[2, 1, 7] == -INF and torch.isfinite(em[2, 1, 7]) and torch.isfinite(a[2, 1]).sum() == M - 1
    # frame 3: three dead particles, and the NaN pose of frame 2 feeds nothing
    for j in (5, 100, 256):
        assert a[3, 1, j] == -INF and em[3, 1, j] == -INF and lw[1, 2, j] == -INF
    assert torch.isfinite(a[3, 1]).sum() == M - 3 and torch.isfinite(lw[1, 2]).sum() == M - 3
    assert lw[1, 1, 7] == -INF and torch.isfinite(lw[1, 1]).sum() == M - 1
    # frame 4: dead -- a row of -inf, -1 and the identity; frame 5 restarts: alpha = emit
    assert (a[4, 1] == -INF).all() and (em[4, 1] == -INF).all()
    assert (lw[1, 3] == -INF).all() and idx[1, 3] == -1 and _bytes_equal(res.R[1, 3], torch.eye(3))
    assert _bytes_equal(a[0, 1], em[0, 1]) and torch.isfinite(a[0, 1]).all()
    assert (idx[1, [0, 1, 2, 4]] >= 0).all()
    # behind the dead frame the backward pass restarts: frame 3 is the log-softmax of its own alpha
    want = torch.log_softmax(a[3, 1].double(), dim=-1)
    fin = torch.isfinite(want)
    assert float((lw[1, 2].double()[fin] - want[fin]).abs().max()) < 1e-5
    # ... and the newest frame that of its emission
    want = torch.log_softmax(em[0, 1].double(), dim=-1)
    assert float((lw[1, 4].double() - want).abs().max()) < 1e-5


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_sample_alone_give_the_same_bytes(ahv, ops, dev):
    M, H = 257, 3
    Rs, scores = _cloud(ahv, M, 3.0, 11, 4)
    rs = np.random.RandomState(3)
    Vs = [(0.05 * rs.standard_normal((B, M, 3))).astype(np.float32) for _ in range(4)]

    def run(rows):
        hist, marg = _chain(ops, dev, H, [R[rows] for R in Rs], [s[rows] for s in scores], 3.0, 8.0, Vs=[V[rows] for V in Vs])
        return marg, ops.marginal_smooth(hist, marg, _step(dev, 4), 3.0)

    (a, pa), (b, pb) = run([0, 1, 2]), run([0, 1, 2])
    for x, y in zip(tuple(a) + tuple(pa), tuple(b) + tuple(pb)):
        assert _bytes_equal(x, y)
    for r in range(B):
        alone, p1 = run([r])
        for x, y in zip(alone, a):
            assert _bytes_equal(x[:, 0], y[:, r]), r
        for x, y in zip(p1, pa):
            assert _bytes_equal(x[0], y[r]), r


def test_ops_refuse_bad_device_arguments(ops, dev):
    M, H = 8, 3
    hist, marg = ops.smooth_history(B, M, H, dev), ops.marginal_history(B, M, H, dev)
    R, s, step = torch.eye(3, device=dev).expand(B, M, 3, 3).contiguous(), torch.zeros(B, M, device=dev), _step(dev, 1)
    ops.smooth_step(hist, R, s, step, 0.02, 3.0)
    ops.marginal_step(hist, marg, R, s, step, 0.02, 3.0)
    ops.marginal_smooth(hist, marg, step, 3.0)
    small = ops.marginal_history(B, M, H + 1, dev)
    bad_out = ops.SmoothedMarginals(torch.empty((B, H, M), device=dev), torch.empty((B, H), dtype=torch.int32, device=dev),
                                    torch.empty((B, H, 3, 3), device=dev))
    for call, word in ((lambda: ops.marginal_step(hist, small, R, s, step, 0.02, 3.0), "marg.alpha"),
                       (lambda: ops.marginal_step(hist, marg._replace(emit=marg.emit.double()), R, s, step, 0.02, 3.0), "marg.emit"),
                       (lambda: ops.marginal_step(hist, marg, R[:, :4].contiguous(), s, step, 0.02, 3.0), "R must be"),
                       (lambda: ops.marginal_step(hist, marg, R, s[:2], step, 0.02, 3.0), "R must be"),
                       (lambda: ops.marginal_step(hist, marg, R, s, step.cpu(), 0.02, 3.0), "no CPU fallback"),
                       (lambda: ops.marginal_step(hist, marg, R, s, step.int(), 0.02, 3.0), "int64"),
                       (lambda: ops.marginal_step(hist, marg, R, s, step, 0.0, 3.0), "temperature"),
                       (lambda: ops.marginal_step(hist, marg, R, s, step, 0.02, 0.0), "sigma_deg"),
                       (lambda: ops.marginal_step(hist, marg, R, s, step, 0.02, 3.0, jump=-1.0), "jump"),
                       (lambda: ops.marginal_smooth(hist, small, step, 3.0), "marg.alpha"),
                       (lambda: ops.marginal_smooth(hist, marg, step, 0.0), "sigma_deg"),
                       (lambda: ops.marginal_smooth(hist, marg, step, 3.0, jump=float("nan")), "jump"),
                       (lambda: ops.marginal_smooth(hist, marg, step, 3.0, frames=0), "frames"),
                       (lambda: ops.marginal_smooth(hist, marg, step, 3.0, frames=H + 1), "frames"),
                       (lambda: ops.marginal_smooth(hist, marg, step, 3.0, out=bad_out), "out must be")):
        with pytest.raises(RuntimeError, match=word):
            call()


# ---- 6. PoseTracker ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(dev):
    g, h = load_golden("batched"), load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    return _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev), w


def _frames(vt, n):
    return [(0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous() for k in range(n)]


def _clone(p):
    return type(p)(*[x.clone() for x in p])


def _trajectory(ahv, dev, pair, steps, **kw):
    """(tracker, [TrackStep clones], [smoothed() clones], [smoothed_marginals() clones or None])"""
    vs, vt, w = pair
    a = dict(particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=1, history=5)
    a.update(kw)
    t = ahv.track.PoseTracker(*w, **a)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    t.init(vs, vt, R0)
    outs, paths, margs = [], [], []
    for f in _frames(vt, steps):
        o = t.step(vs, f)
        outs.append(type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o]))
        paths.append(_clone(t.smoothed()))
        margs.append(_clone(t.smoothed_marginals()) if a.get("marginals") else None)
    return t, outs, paths, margs


NAMES = ("particles", "scores", "draws", "score", "idx", "R_map", "reacquired")


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_marginals_change_no_byte_of_the_tracker(ahv, ops, dev, pair, motion):
    t0, plain, ppaths, _ = _trajectory(ahv, dev, pair, 8, motion=motion)
    t1, with_m, mpaths, margs = _trajectory(ahv, dev, pair, 8, motion=motion, marginals=True)
    for k, (x, y) in enumerate(zip(plain, with_m)):
        for name in NAMES:
            assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (k, name)
    for x, y in zip(ppaths, mpaths):
        assert torch.equal(x.idx, y.idx) and _bytes_equal(x.R, y.R)
    for x, y in zip(t0._hist, t1._hist):
        assert (x is None and y is None) or _bytes_equal(x, y)
    rows = torch.arange(B, device=dev)
    for n, m in enumerate(margs, 1):
        F = min(n, 5)
        assert tuple(m.logw.shape) == (B, F, 257) and (m.idx >= 0).all() and (m.idx < 257).all()
        assert float((m.logw.double().exp().sum(-1) - 1.0).abs().max()) < 1e-4
        for k in range(F):                                               # every frame: a particle of that step
            assert _bytes_equal(m.R[:, -1 - k], with_m[n - 1 - k].particles[rows, m.idx[:, -1 - k]])
    # the newest frame's marginal is the filter's own posterior, and posterior=True returns pose_posterior's numbers
    m, R_mean, spread, mass, entropy = t1.smoothed_marginals(posterior=True)
    assert _bytes_equal(m.logw, margs[-1].logw) and tuple(R_mean.shape) == (B, 5, 3, 3)
    assert tuple(spread.shape) == tuple(mass.shape) == tuple(entropy.shape) == (B, 5)
    slot = 8 % 5
    p = ops.pose_posterior(m.logw[:, -1].contiguous(), t1._hist.R[slot], 1.0, anchors=m.R[:, -1:].contiguous(), min_angle_deg=t1.mode_angle_deg)
    assert float((p.R_mean - R_mean[:, -1]).abs().max()) < 1e-5 and float((p.entropy - entropy[:, -1]).abs().max()) < 1e-4
    assert float((p.mode_prob[:, 0] - mass[:, -1]).abs().max()) < 1e-5
    pd = m.logw.double().exp()
    assert float((entropy.double() + (pd * m.logw.double().clamp_min(-1e30)).sum(-1)).abs().max()) < 1e-3
    assert (mass > 0).all() and (mass <= 1.0 + 1e-6).all()
    assert tuple(t1.smoothed_marginals(frames=2).logw.shape) == (B, 2, 257)


def test_captured_and_eager_marginals_are_the_same_bytes(ahv, ops, dev, pair):
    for motion in ("walk", "constant_velocity"):
        _, eo, ep, em = _trajectory(ahv, dev, pair, 7, motion=motion, marginals=True)
        tg, go, gp, gm = _trajectory(ahv, dev, pair, 7, motion=motion, marginals=True, use_graph=True)
        assert sorted(tg._graphs) == [0, 1]
        for k, (x, y) in enumerate(zip(eo, go)):
            for name in NAMES:
                assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (motion, k, name)
        for k, (x, y) in enumerate(zip(em, gm)):
            assert _bytes_equal(x.logw, y.logw) and torch.equal(x.idx, y.idx) and _bytes_equal(x.R, y.R), (motion, k)


def test_a_step_with_marginals_allocates_nothing(ahv, ops, dev, pair):
    vs, vt, w = pair
    counts = {}
    for marginals in (False, True):
        t = ahv.track.PoseTracker(*w, particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=1, history=5,
                                  marginals=marginals)
        t.init(vs, vt, _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev))
        ring = None
        for n, f in enumerate(_frames(vt, 5), 1):
            before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
            t.step(vs, f)
            after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
            if n >= 3:
                counts.setdefault(marginals, []).append(after - before)
            if marginals:
                here = tuple(x.data_ptr() for x in t._marg)
                assert ring is None or here == ring
                ring = here
    print("allocations per steady-state step: marginals=False %s, marginals=True %s" % (counts[False], counts[True]))
    assert counts[True] == counts[False]                  # the forward step adds no allocation to the step
    # the query into ``out`` allocates nothing either
    out = _clone(t.smoothed_marginals())
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    t.smoothed_marginals(out=out)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before


def test_init_hides_the_old_slots(ahv, ops, dev, pair):
    vs, vt, w = pair
    t, outs, paths, margs = _trajectory(ahv, dev, pair, 6, marginals=True)
    assert tuple(margs[-1].logw.shape) == (B, 5, 257)
    old = [x.clone() for x in t._marg]
    t.init(vs, vt, _t(ahv.rotations.haar_rotations_np(300, seed=6)).to(dev))
    with pytest.raises(RuntimeError, match="before the first step"):
        t.smoothed_marginals()
    for x, y in zip(t._marg, old):
        assert _bytes_equal(x, y)                         # init does not clear the ring
    o = t.step(vs, vt)
    m = t.smoothed_marginals()
    assert tuple(m.logw.shape) == (B, 1, 257)
    assert _bytes_equal(t._marg.alpha[1], t._marg.emit[1])    # frame 1 saw no predecessors, though slot 0 holds frame 5 of the old run
    want = torch.log_softmax(o.scores.double() / 0.05, dim=-1)
    assert float((m.logw[:, 0].double() - want).abs().max()) < 1e-4
    full = ops.marginal_smooth(t._hist, t._marg, t.step_counter, t.smooth_sigma_deg, jump=t.smooth_jump, frames=5)
    assert (full.idx[:, :4] == -1).all() and torch.equal(full.idx[:, 4], m.idx[:, 0]) and (full.logw[:, :4] == -INF).all()
    assert _bytes_equal(full.logw[:, 4], m.logw[:, 0])
    for k in range(4):
        assert _bytes_equal(full.R[:, k], torch.eye(3).expand(B, 3, 3))


# ---- 7. the planted sequence with two distractor frames, on the device ----------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_distractor_on_the_device(ahv, ops, dev, s):
    """smooth_reference.DISTRACTED with the device's noise: the filter's reported pose is more than 90 degrees off on frames 5
    and 8 (the premise); the arg-max of the smoothed marginal and the marginal-weighted mean pose both stay, over frames 4-11,
    below the blind 4 096-hypothesis median of the clean sequence."""
    P = sm.DISTRACTED
    h = load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    vs = _t(h["vol_src"]).to(dev)
    R0 = _t(tr.planted_init(ahv.rotations, s)).to(dev)
    t = ahv.track.PoseTracker(*w, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"], temperature=P["temperature"],
                              batch=1, seed=s, history=P["history"], smooth_sigma_deg=P["smooth_sigma_deg"], smooth_jump=P["smooth_jump"],
                              marginals=True)
    rotate = lambda R: ops.rotate_volume(vs, _t(R[None].astype(np.float32)).to(dev))
    got = {}

    def query():
        got["m"], got["R_mean"], got["spread"], got["mass"], got["entropy"] = t.smoothed_marginals(posterior=True)
        return got["m"]

    filt, arg_err = sm.distracted_run(ahv.rotations, s, rotate, lambda vt: t.init(vs, vt, R0), lambda vt: t.step(vs, vt), query)
    gt = tr.planted_truth(ahv.rotations, s)
    mean_err = tr.geodesic_deg(got["R_mean"][0].double().cpu().numpy(), gt[1:])
    blind = []
    for k in range(P["frames"]):
        Rb = ops.select_rotation(ops.verify_pair(vs, rotate(gt[k]), R0, *w, want_scores=False)[1], R0)[2][0].cpu().numpy()
        blind.append(float(tr.geodesic_deg(Rb.astype(np.float64), gt[k])))
    worst_arg, median = sm.distracted_bar(arg_err, blind)
    worst_mean, _ = sm.distracted_bar(mean_err, blind)
    print("distractor s=%d on the device: filter %s | marginal arg-max (frames 1-11) %s | mean pose %s | max over 4-11: arg-max %.3f, "
          "mean %.3f | blind median %.3f | mode mass %s | spread %s"
          % (s, " ".join("%.2f" % e for e in filt), " ".join("%.2f" % e for e in arg_err), " ".join("%.2f" % e for e in mean_err),
             worst_arg, worst_mean, median, " ".join("%.2f" % e for e in got["mass"][0].cpu()),
             " ".join("%.2f" % e for e in got["spread"][0].cpu())))
    for k in P["distractors"]:
        assert filt[k] > 90.0, (k, filt[k])
    assert worst_arg < median
    assert worst_mean < median
