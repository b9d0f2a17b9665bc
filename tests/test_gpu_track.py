"""Pose tracking on the device: ``ahv_diffuse_rotations_f32`` / ``ahv_track_advance`` against the fp64 reference
(tests/track_reference.py), the noise they draw, and ``track.PoseTracker`` (determinism, the elite's score, the planted moving
optimum, the captured step against the eager one, the posterior outputs).

Shapes: B = 3, N in {1, 5, 1025}, M in {1, 3, 255, 256, 257, 1025} -- one slot, fewer than a lane group, the block edges,
several blocks with a ragged end -- with R shared and per sample.

Figures measured on the MI355X (this file prints them; DESIGN 4.2 quotes them):
  diffused slots against fp64, max |entry| error over all shapes: kernel 4.0e-07, stock fp32 torch composition 2.8e-07 (bar 4 x)
  no drift, max |R^T R - I| after 256 chained calls: 5.7e-07; ops.random_rotations output of the same size: 6.4e-07 (bar 4 x)
  planted moving optimum, tracker max over frames 6-11 / blind median: 1.20 / 8.44, 1.62 / 8.00, 1.37 / 7.01 degrees
"""
import math

import numpy as np
import pytest
import torch

from . import track_reference as tr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
B = 3
NS, MS = (1, 5, 1025), (1, 3, 255, 256, 257, 1025)
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


def _rows(R, idx):
    """R (N,3,3) / (B,N,3,3) host tensor, idx (B,M) -> (B,M,3,3) with the stay-in-bounds rule."""
    return _t(tr.gather(R.numpy(), np.asarray(idx)))


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


# ---- 1. exact slots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True])
def test_elite_and_fresh_slots_are_exact(ahv, ops, dev, per_sample):
    for N in NS:
        R = _set(ahv, N, per_sample)
        Rd = R.to(dev)
        # sample 0: a valid index; sample 1: EMPTY; sample 2: an index outside [0, N) -- both take row 0
        want_idx = np.array([N - 1, 0, 0])
        keys = ahv.dist.pack_keys_host(np.array([0.5, 0.0, 0.25], np.float32), np.array([N - 1, 0, N + 3], np.int64)).copy()
        keys[1] = ahv.dist.KEY_EMPTY
        keys = _t(keys).to(dev)
        elite = _rows(R, want_idx[:, None])[:, 0]
        for M in MS:
            ref = torch.stack([ops.random_rotations(M, seed=SEED ^ tr.FRESH_SEED_XOR, offset=(STEP * B + b) * M, device=dev)
                               for b in range(B)])
            idx = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(M), dtype=torch.int64).to(dev)
            for nf in sorted({0, 1, M}):
                out, om = ops.diffuse_rotations(Rd, idx=idx, sigma_deg=3.0, step=_step(dev), seed=SEED, best_key=keys, n_fresh=nf,
                                                want_omega=True)
                assert torch.equal(out[:, 0].cpu(), elite), (N, M, nf)
                lo = max(M - nf, 1)                      # slot 0 is the elite even when every slot is fresh
                assert torch.equal(out[:, lo:], ref[:, lo:]), (N, M, nf)
                assert not om[:, 0].any() and not om[:, lo:].any()
                if lo > 1:
                    assert om[:, 1:lo].abs().sum(-1).min() > 0      # the diffused slots did move
            # no key: slot 0 is an ordinary slot, and with n_fresh = M every slot is fresh
            out, om = ops.diffuse_rotations(Rd, idx=idx, sigma_deg=3.0, step=_step(dev), seed=SEED, n_fresh=M, want_omega=True)
            assert torch.equal(out, ref) and not om.any()


def test_random_rotations_bytes_are_unchanged(ops, dev):
    """The Haar sampler's body moved into a device function shared with the fresh slots: its output is the bytes recorded from
    the library before that change (tests/golden/random_rotations_recorded.npz)."""
    g = load_golden("random_rotations_recorded")
    for k in ("a", "b"):
        n, seed, offset = (int(v) for v in g[k + "_args"])
        got = ops.random_rotations(n, seed=seed, offset=offset, device=dev)
        assert _bytes_equal(got.cpu(), _t(g[k])), k
        assert torch.equal(got, ops.random_rotations(n, seed=seed, offset=offset, device=dev))


# ---- 2. diffused slots against fp64 --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy(ahv, ops, dev):
    """Every (N, M, layout) case once: the kernel's and the stock fp32 torch composition's max |entry| error against
    track_reference.diffuse in fp64, with the omega the kernel reported.  idx holds -1 and N entries (row 0)."""
    rot = ahv.rotations
    kern = stock = 0.0
    for per_sample in (False, True):
        for N in NS:
            R = _set(ahv, N, per_sample, seed=1)
            for M in MS:
                for sigma in (3.0, 30.0):
                    idx = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(N + M), dtype=torch.int64)
                    idx[0, 0], idx[-1, -1] = -1, N
                    out, om = ops.diffuse_rotations(R.to(dev), idx=idx.to(dev), sigma_deg=sigma, step=_step(dev), seed=SEED,
                                                    want_omega=True)
                    out, om = out.cpu(), om.cpu()
                    want = tr.diffuse(R.double().numpy(), idx.numpy(), om.double().numpy())
                    kern = max(kern, float(np.abs(out.double().numpy() - want).max()))
                    E = rot.axis_angle_to_matrix(om.reshape(-1, 3)).reshape(B, M, 3, 3)          # fp32 on the CPU
                    st = torch.matmul(_rows(R, idx.numpy()), E)
                    stock = max(stock, float(np.abs(st.double().numpy() - want).max()))
    return kern, stock


def test_diffused_slots_match_fp64(accuracy):
    kern, stock = accuracy
    print("diffused slots, max |entry| error against fp64: kernel %.3e, stock fp32 torch composition %.3e" % (kern, stock))
    assert kern <= 4.0 * stock


# ---- 3. noise ------------------------------------------------------------------------------------------------------------
def test_noise_is_standard_normal_and_independent(ahv, ops, dev):
    M, sigma = 4096, 3.0
    R = _set(ahv, 5, True).to(dev)          # per sample: B comes from R
    om = []
    for t in (STEP, STEP + 1):
        om.append(ops.diffuse_rotations(R, m=M, sigma_deg=sigma, step=_step(dev, t), seed=SEED, want_omega=True)[1].cpu().double()
                  .numpy() / math.radians(sigma))
    z, z1 = om[0].reshape(-1, 3), om[1].reshape(-1, 3)
    n = z.size
    assert n == 3 * 4096 * 3
    band, five = dkw(n), 5.0 / math.sqrt(n)      # the issue's n for every bound, the per-component ones included
    gap = ecdf_gap(z.reshape(-1), PHI)
    gaps = [ecdf_gap(z[:, c], PHI) for c in range(3)]
    corr = lambda a, b: abs(float(np.corrcoef(a, b)[0, 1]))
    within = [corr(z[:, a], z[:, b]) for a, b in ((0, 1), (0, 2), (1, 2))]
    across = [corr(z[:, a], z1[:, b]) for a in range(3) for b in range(3)]       # step t against step t + 1, same slots
    print("noise: ECDF gap pooled %.4f, per component %s (band %.4f); mean pooled %.4f, per component %s; correlations between "
          "components %s, between steps at most %.4f (bound %.4f)"
          % (gap, ["%.4f" % x for x in gaps], band, z.mean(), ["%.4f" % x for x in z.mean(0)], ["%.4f" % x for x in within],
             max(across), five))
    assert gap <= band
    assert abs(z.mean()) <= five
    for c in range(3):
        assert gaps[c] <= band
        assert abs(z[:, c].mean()) <= five
        # the spread is left to the test: a component's sample deviation has standard error 1 / sqrt(2 n / 3)
        assert abs(z[:, c].std() - 1.0) <= 5.0 / math.sqrt(2 * n // 3)
    assert max(within) <= five
    assert max(across) <= five


def test_noise_of_a_slot_depends_on_seed_step_b_j_only(ahv, ops, dev):
    R = _set(ahv, 1025, True).to(dev)
    g = torch.Generator().manual_seed(1)
    call = lambda M, idx=None, seed=SEED, t=STEP: ops.diffuse_rotations(
        R, idx=idx, m=None if idx is not None else M, sigma_deg=3.0, step=_step(dev, t), seed=seed, want_omega=True)[1]
    base = call(1025)
    assert torch.equal(call(100), base[:, :100])
    for _ in range(2):
        idx = torch.randint(0, 1025, (B, 1025), generator=g, dtype=torch.int64).to(dev)
        assert torch.equal(call(1025, idx)[:, :100], base[:, :100])
    assert not torch.equal(call(100, seed=SEED + 1), base[:, :100])
    assert not torch.equal(call(100, t=STEP + 1), base[:, :100])
    assert not torch.equal(base[0], base[1])


def test_max_angle_clips_the_step(ahv, ops, dev, accuracy):
    N, M, max_deg = 1025, 1025, 2.0
    R = _set(ahv, N, False)
    idx = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(2), dtype=torch.int64)
    free = ops.diffuse_rotations(R.to(dev), idx=idx.to(dev), sigma_deg=3.0, step=_step(dev), seed=SEED, want_omega=True)[1].cpu()
    out, om = ops.diffuse_rotations(R.to(dev), idx=idx.to(dev), sigma_deg=3.0, step=_step(dev), seed=SEED, max_angle_deg=max_deg,
                                    want_omega=True)
    out, om = out.cpu(), om.cpu()
    bound = float(np.float32(math.radians(max_deg)))                       # what the entry point is given
    norm = np.linalg.norm(om.double().numpy(), axis=-1)
    was = np.linalg.norm(free.double().numpy(), axis=-1)
    assert (was > bound).mean() > 0.5                                       # the limit bites on most slots
    assert norm.max() <= bound
    assert norm[was > bound].min() >= bound * (1 - 1e-5)                    # clipped to the limit, not below it
    inside = was < bound * (1 - 1e-5)
    assert torch.equal(om[_t(inside)], free[_t(inside)])                    # a step inside the limit is untouched
    # the move itself: the fp32 error of the previous test, as an angle (entries off by e: Frobenius 3 e = sqrt(2) angle), for
    # the kernel's output and for the fp32 input row
    tol = math.degrees(2.0 * 3.0 * accuracy[0] / math.sqrt(2.0))
    moved = tr.geodesic_deg(_rows(R, idx.numpy()).double().numpy(), out.double().numpy())
    print("max_angle %.1f deg: largest move %.6f deg, tolerance %.2e deg" % (max_deg, moved.max(), tol))
    assert moved.max() <= math.degrees(bound) + tol


# ---- 4. no drift -------------------------------------------------------------------------------------------------------
def test_chained_diffusion_stays_on_so3(ahv, ops, dev):
    M = 257
    defect = lambda R: float((R.double().transpose(-1, -2) @ R.double() - torch.eye(3, dtype=torch.float64)).abs().max())
    fresh = ops.random_rotations(B * M, seed=3, device=dev).reshape(B, M, 3, 3)
    bufs = [fresh.clone(), torch.empty_like(fresh)]
    step = _step(dev, 0)
    for k in range(256):
        ops.diffuse_rotations(bufs[k & 1], sigma_deg=3.0, step=step, seed=SEED, out=bufs[1 - (k & 1)])
        step += 1
    got, base = defect(bufs[0].cpu()), defect(fresh.cpu())
    print("max |R^T R - I| after 256 chained calls %.3e; random_rotations output of the same size %.3e" % (got, base))
    assert got <= 4.0 * base
    assert float(tr.geodesic_deg(fresh.cpu().numpy(), bufs[0].cpu().numpy()).min()) > 1.0      # (the particles did walk)


# ---- 5. a bad row stays with its slots ------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [False, True])
def test_bad_rows_change_no_other_slot(ahv, ops, dev, per_sample):
    N, M = 5, 257
    R = _set(ahv, N, per_sample)
    bad = R.clone()
    bad[..., 2, :, :] = 0.0
    bad[..., 3, :, :] = float("nan")
    idx = torch.randint(0, N, (B, M), generator=torch.Generator().manual_seed(4), dtype=torch.int64)
    keys = _t(ahv.dist.pack_keys_host(np.full(B, 0.5, np.float32), np.array([0, 1, 4], np.int64))).to(dev)
    run = lambda X: ops.diffuse_rotations(X.to(dev), idx=idx.to(dev), sigma_deg=3.0, step=_step(dev), seed=SEED, best_key=keys,
                                          n_fresh=16, want_omega=True)
    (a, wa), (b, wb) = run(R), run(bad)
    reads_bad = (idx == 2) | (idx == 3)
    reads_bad[:, 0] = False            # the elite rows are clean
    reads_bad[:, M - 16:] = False      # fresh slots read nothing
    clean = ~reads_bad
    assert reads_bad.any()
    assert _bytes_equal(a.cpu()[clean], b.cpu()[clean])
    assert _bytes_equal(wa.cpu(), wb.cpu())                  # the noise never depends on R
    zero = idx == 2
    zero[:, 0] = False
    zero[:, M - 16:] = False
    assert not torch.equal(a.cpu()[zero], b.cpu()[zero])    # (the bad rows did reach their own slots)


# ---- 5b. the op's host checks on device tensors ---------------------------------------------------------------------------
def test_ops_refuse_bad_device_arguments(ahv, ops, dev):
    N, M = 5, 7
    R = _set(ahv, N, True).to(dev)
    idx = torch.zeros((B, M), dtype=torch.int64, device=dev)
    step = _step(dev)
    call = lambda **kw: ops.diffuse_rotations(R, **dict(dict(idx=idx, sigma_deg=3.0, step=step, seed=SEED), **kw))
    call()                                                              # the base call is accepted
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    for kw, word in ((dict(m=M + 1), "disagrees with idx"), (dict(idx=idx.int()), "int64"), (dict(idx=idx[:, ::2]), "contiguous"),
                     (dict(idx=idx.cpu()), "same device"), (dict(idx=idx[:2]), "R must be"), (dict(n_fresh=M + 1), "n_fresh"),
                     (dict(best_key=torch.zeros(B + 1, dtype=torch.int64, device=dev)), "best_key"),
                     (dict(best_key=torch.zeros(B, dtype=torch.int32, device=dev)), "best_key"),
                     (dict(out=f32(B, M + 1, 3, 3)), "out must be"), (dict(out=f32(B, M, 9)), "out must be"),
                     (dict(out=f32(B, M, 3, 3).double()), "out must be"),
                     (dict(omega_out=f32(B, M, 4)), "omega_out must be"), (dict(omega_out=f32(B, M + 1, 3)), "omega_out must be"),
                     (dict(step=step.cpu()), "no CPU fallback"), (dict(step=None), "step is required"),
                     (dict(sigma_deg=float("inf")), "sigma_deg"), (dict(max_angle_deg=-1.0), "max_angle_deg")):
        with pytest.raises(RuntimeError, match=word):
            call(**kw)
    # out / omega_out anywhere inside R's memory, at an offset too
    big = f32(B * N * 9 + B * M * 9)
    Rv = big[:B * N * 9].view(B, N, 3, 3).copy_(R)
    for off in (0, 9, B * N * 9 - 1):
        with pytest.raises(RuntimeError, match="out must not overlap R"):
            ops.diffuse_rotations(Rv, idx=idx, step=step, out=big[off:off + B * M * 9].view(B, M, 3, 3))
    with pytest.raises(RuntimeError, match="omega_out must not overlap R"):
        ops.diffuse_rotations(Rv, idx=idx, step=step, omega_out=big[3:3 + B * M * 3].view(B, M, 3))
    out = big[B * N * 9:].view(B, M, 3, 3)                              # right behind R: accepted
    om = f32(B, M, 3)
    got = ops.diffuse_rotations(Rv, idx=idx, sigma_deg=3.0, step=step, seed=SEED, out=out, omega_out=om)
    assert got[0] is out and got[1] is om
    want = call(want_omega=True)
    assert torch.equal(out, want[0]) and torch.equal(om, want[1])
    with pytest.raises(RuntimeError, match="u must be"):
        ops.track_advance(step, SEED, B, u=f32(B + 1))
    with pytest.raises(RuntimeError, match="u must be"):
        ops.track_advance(step, SEED, B, u=torch.empty(B, dtype=torch.float64, device=dev))
    assert int(step[0]) == STEP                                         # a refused call moved nothing


# ---- 6. track_advance -----------------------------------------------------------------------------------------------------
def test_track_advance(ops, dev):
    calls = 4096
    step = _step(dev, 0)
    buf = torch.empty((calls, B), dtype=torch.float32, device=dev)
    for i in range(calls):
        ops.track_advance(step, SEED, B, u=buf[i])
    assert int(step[0]) == calls                                     # one per call
    u = buf.cpu().double().numpy()
    assert u.min() >= 0.0 and u.max() < 1.0
    gap0, gap = ecdf_gap(u[:, 0], lambda v: v), ecdf_gap(u.reshape(-1), lambda v: v)
    print("track_advance: ECDF gap of sample 0 over %d calls %.4f (band %.4f), pooled %.4f (band %.4f)"
          % (calls, gap0, dkw(calls), gap, dkw(u.size)))
    assert gap0 <= dkw(calls) and gap <= dkw(u.size)
    # a function of (seed, step, b): a second run, and a run at another batch size, agree on the common samples
    step2 = _step(dev, 0)
    wide = torch.stack([ops.track_advance(step2, SEED, 7) for _ in range(8)])
    assert int(step2[0]) == 8 and torch.equal(wide[:, :B], buf[:8])
    step3 = _step(dev, 5)
    assert torch.equal(ops.track_advance(step3, SEED, B), buf[5]) and int(step3[0]) == 6
    assert not torch.equal(ops.track_advance(_step(dev, 5), SEED + 1, B), buf[5])
    big = ops.track_advance(_step(dev, 5), SEED, 1000)                # more samples than one pass of the workgroup
    assert torch.equal(big[:B], buf[5]) and float(big.min()) >= 0.0 and float(big.max()) < 1.0


# ---- 7. PoseTracker ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(dev):
    g, h = load_golden("batched"), load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    return _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev), w


def _frames(vt, n):
    """n target volumes from the fixture's: its samples rolled and blended, so that every frame differs."""
    return [(0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous() for k in range(n)]


def _tracker(ahv, w, seed=1, **kw):
    a = dict(particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=seed)
    a.update(kw)
    return ahv.track.PoseTracker(*w, **a)


def _trajectory(ahv, dev, pair, steps=4, **kw):
    vs, vt, w = pair
    t = _tracker(ahv, w, **kw)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    outs = [t.init(vs, vt, R0)]
    for f in _frames(vt, steps):
        o = t.step(vs, f)
        outs.append(type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o]))
    return outs


def test_same_seed_same_bytes(ahv, ops, dev, pair):
    a, b, c = (_trajectory(ahv, dev, pair, seed=s) for s in (1, 1, 2))
    for x, y in zip(a[1:], b[1:]):
        for name in ("particles", "scores", "draws", "score", "idx", "R_map", "reacquired"):
            assert torch.equal(getattr(x, name), getattr(y, name)), name
    assert not torch.equal(a[1].particles, c[1].particles)


def test_elite_score_is_the_scorers(ahv, ops, dev, pair):
    vs, vt, w = pair
    outs = _trajectory(ahv, dev, pair)
    for k, f in enumerate(_frames(vt, 4)):
        prev, cur = outs[k], outs[k + 1]
        assert torch.equal(cur.particles[:, 0], prev.R_map)
        ft = ops.verify_pair(vs, f, cur.particles[:, :1].contiguous(), *w, want_feat_tgt=True)[2]   # the in-launch features
        want = ops.score_hypotheses(vs, ft, prev.R_map[:, None].contiguous(), *w)[0][:, 0]
        assert torch.equal(cur.scores[:, 0], want)
        assert (cur.score >= cur.scores[:, 0]).all()
        assert torch.equal(cur.score, cur.scores.max(dim=1).values)
        assert torch.equal(cur.reacquired, cur.idx >= 257 - 8)


@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_moving_optimum_on_the_device(ahv, ops, dev, s):
    P = tr.PLANTED
    h = load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    vs = _t(h["vol_src"]).to(dev)
    R0 = _t(tr.planted_init(ahv.rotations, s)).to(dev)

    class T:
        def __init__(self):
            self.t = ahv.track.PoseTracker(*w, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                           temperature=P["temperature"], batch=1, seed=s)

        def init_frame(self, vt):
            return self.t.init(vs, vt, R0)

        def step_frame(self, vt):
            return self.t.step(vs, vt)

    rotate = lambda R: ops.rotate_volume(vs, _t(R[None].astype(np.float32)).to(dev))
    blind = lambda vt: ops.select_rotation(ops.verify_pair(vs, vt, R0, *w, want_scores=False)[1], R0)[2][0].cpu().numpy()
    track, blind_err = tr.planted_run(ahv.rotations, s, rotate, T, blind)
    worst, median = tr.planted_bar(track, blind_err)
    print("planted s=%d on the device: tracker %s | late max %.3f | blind median %.3f"
          % (s, " ".join("%.2f" % e for e in track), worst, median))
    assert worst < median


def test_captured_steps_equal_eager_steps(ahv, ops, dev, pair):
    vs, vt, w = pair
    steps = 6
    eager = _trajectory(ahv, dev, pair, steps=steps, posterior=True)
    graphed = _trajectory(ahv, dev, pair, steps=steps, posterior=True, use_graph=True)
    for k, (x, y) in enumerate(zip(eager, graphed)):
        for name in ("particles", "scores", "score", "idx", "R_map", "reacquired", "R_mean", "spread_deg", "mode_mass", "entropy"):
            assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (k, name)
        if k:
            assert torch.equal(x.draws, y.draws), k
    # the static inputs: write the volumes there and replay with no arguments
    t = _tracker(ahv, w, use_graph=True)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    t.init(vs, vt, R0)
    for k, f in enumerate(_frames(vt, steps)):
        t.buffers[0].copy_(vs)
        t.buffers[1].copy_(f)
        o = t.step()
        assert torch.equal(o.particles, eager[k + 1].particles) and torch.equal(o.scores, eager[k + 1].scores), k
    assert sorted(t._graphs) == [0, 1]


def test_posterior_outputs_are_pose_posteriors(ahv, ops, dev, pair):
    vs, vt, w = pair
    t = _tracker(ahv, w, posterior=True, mode_angle_deg=10.0)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    outs = [t.init(vs, vt, R0)] + [t.step(vs, f) for f in _frames(vt, 2)][-1:]
    for o in outs:
        p = ops.pose_posterior(o.scores, o.particles, 0.05, anchors=o.R_map[:, None].contiguous(), min_angle_deg=10.0)
        assert torch.equal(o.mode_mass, p.mode_prob[:, 0]) and torch.equal(o.R_mean, p.R_mean)
        assert torch.equal(o.entropy, p.entropy) and torch.equal(o.spread_deg, p.spread_deg)
        assert ((o.mode_mass > 0) & (o.mode_mass <= 1)).all()
