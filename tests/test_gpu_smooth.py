"""Trajectory smoothing on the device: ``ahv_smooth_step_f32`` / ``ahv_smooth_backtrace_f32`` against the fp64 reference
(tests/smooth_reference.py) and ``track.PoseTracker(history=H)``.

Shapes: B = 3, M in {1, 2, 63, 64, 65, 257, 1025} -- one particle, fewer than a workgroup's 16 successors, a ragged last
workgroup (63 = 3 x 16 + 15, 65 = 4 x 16 + 1) beside a full one, a ragged predecessor tile (257 = 256 + 1) and several tiles with
many workgroups -- and H in {2, 3, 5}.

Figures measured on the MI355X (this file prints them; DESIGN 4.2 quotes them):
  delta against fp64, max over all M (kernel / stock fp32 torch composition; bar 4 x): 1.9e-06 / 1.9e-06 at jump 0 (the rounding
  of the stored fp32 alone), 2.4e-06 / 3.9e-06 at sigma 3 deg and 2.2e-06 / 3.7e-06 at 30 deg with jump 8 and +inf, 2.2e-06 /
  3.9e-06 and 2.2e-06 / 4.0e-06 with velocities; the fp64 shortfall of the chosen predecessor is 0 in every configuration
  hist_P against fp64 R exp(damping v): kernel 3.8e-07 / stock 1.2e-07 at sigma 3 deg, 3.7e-07 / 2.0e-07 at 30 deg (bar 4 x)
  planted distractor, filter error on frames 5 / 8, then smoothed max over frames 4-11 / blind median, degrees:
  167.8 / 107.9, 3.00 / 8.44; 144.1 / 134.4, 4.13 / 8.00; 157.0 / 115.9, 2.62 / 7.01
"""
import math

import numpy as np
import pytest
import torch

from . import smooth_reference as sm
from . import track_reference as tr
from .conftest import load_golden

pytestmark = pytest.mark.gpu
B = 3
MS, HS = (1, 2, 63, 64, 65, 257, 1025), (2, 3, 5)
INF = float("inf")
ONE_RAD_DEG = math.degrees(1.0)


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


def _nan_ring(ops, dev, nb, M, H, velocities=False):
    """A ring whose every word is the NaN pattern 0x7FC00000 (as an index: far outside [0, M))."""
    h = ops.smooth_history(nb, M, H, dev, velocities=velocities)
    for x in h:
        if x is not None:
            x.view(torch.int32).fill_(0x7FC00000)
    return h


# ---- 1. the exact lattice ------------------------------------------------------------------------------------------------
def cube_rotations():
    """The 24 rotations of the cube: signed permutation matrices of determinant +1."""
    out = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in range(8):
            Q = np.zeros((3, 3))
            for r in range(3):
                Q[r, p[r]] = -1.0 if sg >> r & 1 else 1.0
            if np.linalg.det(Q) > 0:
                out.append(Q)
    assert len(out) == 24
    return np.stack(out)


def lattice(M, frames, seed, nb=B):
    """frames sets (nb,M,3,3) of cube rotations with repeats and scores (nb,M) in multiples of 2^-6 with many ties: with sigma = 1
    rad (1/(4 sigma^2) = 1/4), T = 1 and jump = 2 every operation of the recursion is exact in fp32."""
    rs = np.random.RandomState(seed)
    C = cube_rotations()
    Rs = [C[rs.randint(0, 24, (nb, M))].astype(np.float32) for _ in range(frames)]
    scores = [(rs.randint(-8, 9, (nb, M)) / 64.0).astype(np.float32) for _ in range(frames)]
    return Rs, scores


def _lattice_chain(ops, dev, M, H, Rs, scores, first_step=1, hist=None, nb=B, check=None):
    """Run the chain on the device into a NaN-filled ring; ``check(f, t, hist)`` after every step."""
    hist = _nan_ring(ops, dev, nb, M, H) if hist is None else hist
    for f, (R, s) in enumerate(zip(Rs, scores)):
        t = first_step + f
        ops.smooth_step(hist, _t(R).to(dev), _t(s).to(dev), _step(dev, t), 1.0, ONE_RAD_DEG, jump=2.0, first_step=first_step)
        if check is not None:
            check(f, t, hist)
    return hist


@pytest.fixture(scope="module")
def lattice_reference():
    """M -> (Rs, scores, [(delta (B,M) fp32, back (B,M)) per frame]): the fp64 recursion, once per M (it does not depend on H)."""
    out = {}
    for M in MS:
        Rs, scores = lattice(M, 7, 100 + M)
        ring = sm.Ring(8, B, M)
        per = []
        for f in range(7):
            ring.step(f + 1, Rs[f], scores[f], 1.0, 1.0, 2.0)
            per.append((ring.delta[(f + 1) % 8].astype(np.float32), ring.back[(f + 1) % 8].copy()))
        out[M] = (Rs, scores, per)
    return out


@pytest.mark.parametrize("H", HS)
def test_exact_lattice_equals_fp64_bit_for_bit(ops, dev, lattice_reference, H):
    for M in MS:
        Rs, scores, per = lattice_reference[M]
        ties = 0

        def check(f, t, hist):
            slot = t % H
            want_d, want_b = per[f]
            assert _bytes_equal(hist.delta[slot], _t(want_d)), (M, H, f)
            assert torch.equal(hist.back[slot].cpu(), _t(want_b)), (M, H, f)
            assert _bytes_equal(hist.R[slot], _t(Rs[f])), (M, H, f)

        hist = _lattice_chain(ops, dev, M, H, Rs, scores, check=check)
        # ties go to the lowest index: the reference's arg-max is the first one, and the lattice has ties
        if M >= 63:
            for f in range(1, 7):
                c, _ = sm.candidates(Rs[f][0], Rs[f - 1][0], per[f - 1][0][0], 0.25, 2.0)
                ties += int(((c == c.max(axis=0)).sum(axis=0) > 1).sum())
            assert ties > 0, (M, ties)
        # the ring wrapped: H < 7 frames, and the slots hold the newest H frames
        for k in range(H):
            assert _bytes_equal(hist.R[(7 - k) % H], _t(Rs[6 - k]))


def test_ties_go_to_the_lowest_index(ops, dev):
    """Equal predecessors: the first one wins, wherever the tied ones sit -- in one wave's rows, in the rows of two waves of a
    tile, in two tiles, and behind better-placed but worse predecessors."""
    C = cube_rotations()
    for M, tied in ((64, range(64)), (257, (200, 256)), (257, (256,)), (257, (37, 38, 100, 255)), (1025, (63, 64, 300, 1024)),
                    (1025, (700, 900)), (65, (64,)), (2, (1,)), (2, (0, 1))):
        R = np.broadcast_to(C[5], (B, M, 3, 3)).astype(np.float32)
        s0 = np.full((B, M), -0.25, np.float32)
        s0[:, list(tied)] = 0.5
        s1 = np.zeros((B, M), np.float32)
        hist = _lattice_chain(ops, dev, M, 2, [R, R], [s0, s1])
        assert (hist.back[0] == min(tied)).all(), (M, tuple(tied), hist.back[0, 0, :4])
        assert _bytes_equal(hist.delta[0], torch.zeros(B, M))


def test_lattice_path_equals_brute_force(ops, dev):
    M, frames = 3, 4
    for seed in range(6):
        Rs, scores = lattice(M, frames, 40 + seed)
        for H in (4, 5):
            hist = _lattice_chain(ops, dev, M, H, Rs, scores)
            path = ops.smooth_backtrace(hist, _step(dev, frames), frames=frames)
            for b in range(B):
                value, paths = sm.brute_force([R[b] for R in Rs], [R[b] for R in Rs], [s[b] for s in scores], 1.0, 0.25, 2.0)
                got = tuple(int(j) for j in path.idx[b].cpu())
                assert got in paths, (seed, b, got, paths)
                for f, j in enumerate(got):
                    assert _bytes_equal(path.R[b, f], _t(Rs[f][b, j]))


# ---- 2. generic inputs against fp64 ------------------------------------------------------------------------------------------
def _cloud(ahv, M, sigma_deg, seed, frames=3):
    """frames sets (B,M,3,3) fp32: a Haar pose per sample, every particle diffused by sigma; scores (B,M) in [-1, 1]."""
    rs = np.random.RandomState(seed)
    base = ahv.rotations.haar_rotations_np(B, seed=seed).astype(np.float64)
    Rs = [(base[:, None] @ tr.exp_so3(math.radians(sigma_deg) * rs.standard_normal((B, M, 3)))).astype(np.float32) for _ in range(frames)]
    scores = [rs.uniform(-1, 1, (B, M)).astype(np.float32) for _ in range(frames)]
    return Rs, scores


def _stock_step(R, s, P_prev, d_prev, beta, k, jump):
    """The stock fp32 torch composition on the host: difference form, clamp, add, max -- an M x M x 9 tensor per sample."""
    diff = P_prev[:, :, None].reshape(B, -1, 1, 9) - R[:, None].reshape(B, 1, -1, 9)
    w = -(diff * diff).sum(-1) * float(np.float32(k))
    w = torch.clamp(w, min=-jump)
    m = d_prev.max(dim=1, keepdim=True).values
    c = (d_prev - m)[:, :, None] + w
    best, idx = c.max(dim=1)
    return float(beta) * s + best, idx


@pytest.fixture(scope="module")
def accuracy(ahv, ops, dev):
    """Per (sigma, jump, velocities) configuration, pooled over every M: the largest |delta - fp64| of the kernel and of the stock
    fp32 composition on the same inputs (the third frame of a chain: its predecessors' deltas are the device's own, fed to all
    three), and the largest fp64 shortfall of the candidate the kernel chose against the fp64 maximum."""
    T = 0.02
    beta = ops.inverse_temperature(T)
    out = {}
    for sigma_deg in (3.0, 30.0):
        for jump in (0.0, 8.0, INF):
            for vel in (False, True):
                if vel and jump != 8.0:
                    continue
                kern = stock = gap = p_kern = p_stock = 0.0
                for M in MS:
                    Rs, scores = _cloud(ahv, M, sigma_deg, 7 * M + int(sigma_deg))
                    rs = np.random.RandomState(M)
                    Vs = [(math.radians(sigma_deg) * rs.standard_normal((B, M, 3))).astype(np.float32) for _ in range(3)] if vel else [None] * 3
                    hist = _nan_ring(ops, dev, B, M, 3, velocities=vel)
                    for f in range(3):
                        ops.smooth_step(hist, _t(Rs[f]).to(dev), _t(scores[f]).to(dev), _step(dev, f + 1), T, sigma_deg, jump=jump,
                                        V=_t(Vs[f]).to(dev) if vel else None, damping=0.9)
                    P_prev = (hist.P if vel else hist.R)[2].cpu()
                    d_prev, got_d, got_b = hist.delta[2].cpu(), hist.delta[0].cpu().double().numpy(), hist.back[0].cpu().numpy()
                    k = sm.inv4s2(ops._angle_rad(sigma_deg, "sigma_deg"))
                    st_d, _ = _stock_step(_t(Rs[2]), _t(scores[2]), P_prev, d_prev, beta, k, jump)
                    for b in range(B):
                        c, _ = sm.candidates(Rs[2][b], P_prev[b].numpy(), d_prev[b].numpy(), k, jump)
                        want_d = beta * scores[2][b].astype(np.float64) + c.max(axis=0)      # (viterbi_step's value: checked below)
                        if M <= 65:
                            assert np.array_equal(want_d, sm.viterbi_step(Rs[2][b], scores[2][b], beta, k, jump, P_prev[b].numpy(),
                                                                          d_prev[b].numpy())[0])
                        assert np.isfinite(want_d).all() and (got_b[b] >= 0).all() and (got_b[b] < M).all()
                        kern = max(kern, float(np.abs(got_d[b] - want_d).max()))
                        stock = max(stock, float(np.abs(st_d[b].double().numpy() - want_d).max()))
                        gap = max(gap, float((c.max(axis=0) - c[got_b[b], np.arange(M)]).max()))
                    if vel:
                        want_P = sm.predicted(Rs[2], Vs[2], 0.9)
                        p_kern = max(p_kern, float(np.abs(hist.P[0].cpu().double().numpy() - want_P).max()))
                        E = ahv.rotations.axis_angle_to_matrix((np.float32(0.9) * _t(Vs[2])).reshape(-1, 3)).reshape(B, M, 3, 3)
                        p_stock = max(p_stock, float(np.abs(torch.matmul(_t(Rs[2]), E).double().numpy() - want_P).max()))
                out[(sigma_deg, jump, vel)] = (kern, stock, gap, p_kern, p_stock)
    return out


def test_generic_delta_and_back_match_fp64(accuracy):
    """Bar: 4 x the error of the stock fp32 torch composition on the same inputs (the project's convention), per configuration."""
    for (sigma_deg, jump, vel), (kern, stock, gap, _, _) in sorted(accuracy.items()):
        print("smooth_step sigma %4.1f deg, jump %4s, velocities %d: max |delta - fp64| kernel %.3e, stock fp32 torch %.3e; fp64 "
              "shortfall of the chosen predecessor %.3e" % (sigma_deg, jump, vel, kern, stock, gap))
    for key, (kern, stock, gap, _, _) in accuracy.items():
        assert kern <= 4.0 * stock, key
        assert gap <= 4.0 * stock, key


def test_predicted_poses_match_fp64(accuracy):
    """hist_P against fp64 R exp(damping v); bar: 4 x the stock fp32 torch composition (axis_angle_to_matrix, matmul)."""
    for (sigma_deg, jump, vel), (_, _, _, p_kern, p_stock) in sorted(accuracy.items()):
        if vel:
            print("hist_P sigma %4.1f deg: max |entry - fp64| kernel %.3e, stock fp32 torch %.3e" % (sigma_deg, p_kern, p_stock))
            assert 0.0 < p_kern <= 4.0 * p_stock


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------
def test_bad_values_stay_with_their_sample(ops, dev):
    """Six samples on the exact lattice, five frames, H = 5; sample 0 is the control.  At frame 3: sample 1 a NaN score, sample 2
    a -inf score, sample 3 a +inf score, sample 5 every score NaN; sample 4 has a NaN matrix row in frame 2, a predecessor of
    frame 3.  Everything equals the fp64 reference bit for bit, and the control's bytes are those of the clean run."""
    M, H, nb, frames = 65, 5, 6, 5
    Rs, scores = lattice(M, frames, 7, nb=nb)
    clean = _lattice_chain(ops, dev, M, H, Rs, scores, nb=nb)
    clean_path = ops.smooth_backtrace(clean, _step(dev, frames))
    Rs, scores = [R.copy() for R in Rs], [s.copy() for s in scores]
    scores[2][1, 5], scores[2][2, 64], scores[2][3, 0] = np.nan, -np.inf, np.inf
    scores[2][5, :] = np.nan
    Rs[1][4, 7] = np.nan
    ring = sm.Ring(H, nb, M)

    def check(f, t, hist):
        ring.step(t, Rs[f], scores[f], 1.0, 1.0, 2.0)
        assert _bytes_equal(hist.delta[t % H], _t(ring.delta[t % H].astype(np.float32))), f
        assert torch.equal(hist.back[t % H].cpu(), _t(ring.back[t % H])), f

    hist = _lattice_chain(ops, dev, M, H, Rs, scores, nb=nb, check=check)
    path = ops.smooth_backtrace(hist, _step(dev, frames))
    want_idx, _ = ring.backtrace(frames, H)
    assert torch.equal(path.idx.cpu(), _t(want_idx))
    for x, y in zip(hist, clean):
        if x is not None:
            assert _bytes_equal(x[:, 0], y[:, 0])                 # the control
    assert torch.equal(path.idx[0], clean_path.idx[0]) and _bytes_equal(path.R[0], clean_path.R[0])
    d3, b3 = hist.delta[3 % H].cpu(), hist.back[3 % H].cpu()
    for b, j in ((1, 5), (2, 64), (3, 0)):                        # dead particles; the rest of the sample lives on
        assert d3[b, j] == -INF and b3[b, j] == -1
        assert torch.isfinite(d3[b]).sum() == M - 1 and (b3[b] >= 0).sum() == M - 1
        assert not (hist.back[4 % H][b].cpu() == j).any()          # nothing descends from a dead particle
        assert (path.idx[b] >= 0).all()
    assert not (b3[4] == 7).any() and torch.isfinite(d3[4]).all() and (b3[4] >= 0).all()      # the NaN row is no candidate
    assert hist.back[2 % H][4, 7] == -1 and torch.isfinite(hist.delta[2 % H][4, 7])           # ... and has none itself
    assert (d3[5] == -INF).all() and (b3[5] == -1).all()
    assert (hist.back[4 % H][5] == -1).all() and torch.isfinite(hist.delta[4 % H][5]).all()   # frame 4 restarts
    # the backtrace restarts behind the break: frames 1..5 -> columns 0..4
    p5 = path.idx[5].cpu()
    assert p5[2] == -1 and _bytes_equal(path.R[5, 2], torch.eye(3)) and (p5[[0, 1, 3, 4]] >= 0).all()
    assert p5[1] == int(np.argmax(ring.delta[2 % H, 5]))          # frame 2: that frame's own first arg-max
    assert p5[0] == ring.back[2 % H, 5, p5[1]]


# ---- 4. the ring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
def test_ring_slots_and_first_step(ops, dev, H):
    M = 65
    first = (1 << 33) + 4
    Rs, scores = lattice(M, 2, 9)
    hist = _nan_ring(ops, dev, B, M, H)
    pattern = torch.full((B, M), 0x7FC00000, dtype=torch.int32)
    ops.smooth_step(hist, _t(Rs[0]).to(dev), _t(scores[0]).to(dev), _step(dev, first), 1.0, ONE_RAD_DEG, jump=2.0, first_step=first)
    s0 = first % H
    # the frame at first_step reads nothing of the NaN-filled ring: delta = beta s, no back pointers
    assert _bytes_equal(hist.delta[s0], _t(scores[0])) and (hist.back[s0] == -1).all() and _bytes_equal(hist.R[s0], _t(Rs[0]))
    for k in range(H):
        if k != s0:
            assert torch.equal(hist.delta[k].view(torch.int32).cpu(), pattern) and torch.equal(hist.back[k].cpu(), pattern)
    ops.smooth_step(hist, _t(Rs[1]).to(dev), _t(scores[1]).to(dev), _step(dev, first + 1), 1.0, ONE_RAD_DEG, jump=2.0, first_step=first)
    s1 = (first + 1) % H                                          # int64 slot arithmetic: 2^33 + 5 is not 5
    assert s1 != 5 % H or H == 2
    ring = sm.Ring(H, B, M)
    ring.step(first, Rs[0], scores[0], 1.0, 1.0, 2.0, first_step=first)
    ring.step(first + 1, Rs[1], scores[1], 1.0, 1.0, 2.0, first_step=first)
    assert _bytes_equal(hist.delta[s1], _t(ring.delta[s1].astype(np.float32))) and torch.equal(hist.back[s1].cpu(), _t(ring.back[s1]))
    assert _bytes_equal(hist.R[s1], _t(Rs[1]))
    for k in range(H):
        if k not in (s0, s1):
            assert torch.equal(hist.delta[k].view(torch.int32).cpu(), pattern)
    # F larger than the two recorded frames: -1 / identity for what was never recorded
    path = ops.smooth_backtrace(hist, _step(dev, first + 1), frames=H, first_step=first)
    want_idx, want_R = ring.backtrace(first + 1, H, first_step=first)
    assert torch.equal(path.idx.cpu(), _t(want_idx)) and _bytes_equal(path.R, _t(want_R.astype(np.float32)))
    assert (path.idx[:, :H - 2] == -1).all() and (path.idx[:, H - 2:] >= 0).all()
    for f in range(H - 2):
        assert _bytes_equal(path.R[:, f], torch.eye(3).expand(B, 3, 3))
    # a step with the same counter but first_step = t again has no predecessors, whatever the ring holds
    ops.smooth_step(hist, _t(Rs[1]).to(dev), _t(scores[1]).to(dev), _step(dev, first + 1), 1.0, ONE_RAD_DEG, jump=2.0, first_step=first + 1)
    assert _bytes_equal(hist.delta[s1], _t(scores[1])) and (hist.back[s1] == -1).all()
    out = ops.SmoothedPath(torch.empty((B, 1), dtype=torch.int64, device=dev), torch.empty((B, 1, 3, 3), device=dev))
    got = ops.smooth_backtrace(hist, _step(dev, first + 1), frames=1, first_step=first + 1, out=out)
    assert got.idx.data_ptr() == out.idx.data_ptr() and got.R.data_ptr() == out.R.data_ptr()
    assert np.array_equal(out.idx[:, 0].cpu().numpy(), scores[1].argmax(axis=1))


def test_ops_refuse_bad_device_arguments(ops, dev):
    M, H = 8, 3
    hist, histv = ops.smooth_history(B, M, H, dev), ops.smooth_history(B, M, H, dev, velocities=True)
    R, s, step = torch.eye(3, device=dev).expand(B, M, 3, 3).contiguous(), torch.zeros(B, M, device=dev), _step(dev, 1)
    V = torch.zeros(B, M, 3, device=dev)
    ops.smooth_step(hist, R, s, step, 0.02, 3.0)
    ops.smooth_step(histv, R, s, step, 0.02, 3.0, V=V)
    for call, word in ((lambda: ops.smooth_step(hist, R, s, step, 0.02, 3.0, V=V), "go together"),
                       (lambda: ops.smooth_step(histv, R, s, step, 0.02, 3.0), "go together"),
                       (lambda: ops.smooth_step(hist, R[:, :4].contiguous(), s, step, 0.02, 3.0), "R must be"),
                       (lambda: ops.smooth_step(hist, R, s[:2], step, 0.02, 3.0), "R must be"),
                       (lambda: ops.smooth_step(histv, R, s, step, 0.02, 3.0, V=V[:, :, :2]), "V must be"),
                       (lambda: ops.smooth_step(hist, R, s, step.cpu(), 0.02, 3.0), "no CPU fallback"),
                       (lambda: ops.smooth_step(hist, R, s, step.int(), 0.02, 3.0), "int64"),
                       (lambda: ops.smooth_step(hist, R.double(), s, step, 0.02, 3.0), "float32"),
                       (lambda: ops.smooth_step(hist, R, s, step, 0.0, 3.0), "temperature"),
                       (lambda: ops.smooth_step(hist, R, s, step, 0.02, 0.0), "sigma_deg"),
                       (lambda: ops.smooth_step(hist, R, s, step, 0.02, INF), "sigma_deg"),
                       (lambda: ops.smooth_step(hist, R, s, step, 0.02, 3.0, jump=-1.0), "jump"),
                       (lambda: ops.smooth_step(hist, R, s, step, 0.02, 3.0, damping=1.5), "damping"),
                       (lambda: ops.smooth_step(hist._replace(back=hist.back.long()), R, s, step, 0.02, 3.0), "history.back"),
                       (lambda: ops.smooth_step(hist._replace(delta=hist.delta[:2]), R, s, step, 0.02, 3.0), "history.delta"),
                       (lambda: ops.smooth_backtrace(hist, step, frames=0), "frames"),
                       (lambda: ops.smooth_backtrace(hist, step, frames=H + 1), "frames"),
                       (lambda: ops.smooth_backtrace(hist, step, out=ops.SmoothedPath(torch.empty((B, H), dtype=torch.int32, device=dev),
                                                                                     torch.empty((B, H, 3, 3), device=dev))), "out must be")):
        with pytest.raises(RuntimeError, match=word):
            call()


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_sample_alone_give_the_same_bytes(ahv, ops, dev):
    M, H, T = 257, 3, 0.02
    Rs, scores = _cloud(ahv, M, 3.0, 11, frames=4)
    rs = np.random.RandomState(3)
    Vs = [(0.05 * rs.standard_normal((B, M, 3))).astype(np.float32) for _ in range(4)]

    def run(rows):
        nb = len(rows)
        hist = _nan_ring(ops, dev, nb, M, H, velocities=True)
        for f in range(4):
            ops.smooth_step(hist, _t(Rs[f][rows]).to(dev), _t(scores[f][rows]).to(dev), _step(dev, f + 1), T, 3.0, V=_t(Vs[f][rows]).to(dev),
                            damping=0.9)
        return hist, ops.smooth_backtrace(hist, _step(dev, 4))

    (a, pa), (b, pb) = run([0, 1, 2]), run([0, 1, 2])
    for x, y in zip(tuple(a) + tuple(pa), tuple(b) + tuple(pb)):
        assert _bytes_equal(x, y)
    for r in range(B):
        alone, p1 = run([r])
        for x, y in zip(alone, a):
            assert _bytes_equal(x[:, 0], y[:, r]), r
        assert torch.equal(p1.idx[0], pa.idx[r]) and _bytes_equal(p1.R[0], pa.R[r])


# ---- 6. PoseTracker ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(dev):
    g, h = load_golden("batched"), load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    return _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev), w


def _frames(vt, n):
    return [(0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous() for k in range(n)]


def ops_path(p):
    return type(p)(p.idx.clone(), p.R.clone())


def _trajectory(ahv, dev, pair, steps, **kw):
    """(tracker, [TrackStep clones], [smoothed() clones or None])"""
    vs, vt, w = pair
    a = dict(particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=1)
    a.update(kw)
    t = ahv.track.PoseTracker(*w, **a)
    R0 = _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev)
    t.init(vs, vt, R0)
    outs, paths = [], []
    for f in _frames(vt, steps):
        o = t.step(vs, f)
        outs.append(type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o]))
        paths.append(ops_path(t.smoothed()) if a.get("history") else None)
    return t, outs, paths


NAMES = ("particles", "scores", "draws", "score", "idx", "R_map", "reacquired")


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_history_changes_no_trackstep_byte(ahv, ops, dev, pair, motion):
    _, plain, _ = _trajectory(ahv, dev, pair, 8, motion=motion)
    t, smooth, paths = _trajectory(ahv, dev, pair, 8, motion=motion, history=5)
    for k, (x, y) in enumerate(zip(plain, smooth)):
        for name in NAMES:
            assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (k, name)
    assert (t._hist.P is not None) == (motion != "walk")
    for n, p in enumerate(paths, 1):
        F = min(n, 5)
        assert tuple(p.idx.shape) == (B, F) and (p.idx >= 0).all() and (p.idx < 257).all()
        rows = torch.arange(B, device=dev)
        assert _bytes_equal(p.R[:, -1], smooth[n - 1].particles[rows, p.idx[:, -1]])      # the newest frame: a particle of the step
        for k in range(1, F):                                                                 # older frames: that step's particles
            assert _bytes_equal(p.R[:, -1 - k], smooth[n - 1 - k].particles[rows, p.idx[:, -1 - k]])
    # the fixed-lag pose and a shorter window are views of the same path
    assert torch.equal(t.smoothed(frames=2).idx, paths[-1].idx[:, -2:])


def test_captured_and_eager_smoothed_paths_are_the_same_bytes(ahv, ops, dev, pair):
    for motion in ("walk", "constant_velocity"):
        _, eo, ep = _trajectory(ahv, dev, pair, 7, motion=motion, history=5)
        tg, go, gp = _trajectory(ahv, dev, pair, 7, motion=motion, history=5, use_graph=True)
        assert sorted(tg._graphs) == [0, 1]
        for k, (x, y) in enumerate(zip(eo, go)):
            for name in NAMES:
                assert _bytes_equal(getattr(x, name).float(), getattr(y, name).float()), (motion, k, name)
        for k, (x, y) in enumerate(zip(ep, gp)):
            assert torch.equal(x.idx, y.idx) and _bytes_equal(x.R, y.R), (motion, k)


def test_a_step_with_history_allocates_nothing(ahv, ops, dev, pair):
    vs, vt, w = pair
    counts = {}
    for history in (0, 5):
        t = ahv.track.PoseTracker(*w, particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=B, seed=1, history=history)
        t.init(vs, vt, _t(ahv.rotations.haar_rotations_np(300, seed=5)).to(dev))
        ptrs, ring = {}, None
        for n, f in enumerate(_frames(vt, 5), 1):
            before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
            out = t.step(vs, f)
            after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
            now = tuple(x.data_ptr() for x in (out.score, out.idx, out.R_map, out.particles, out.scores, out.draws, out.reacquired))
            if n >= 3:
                assert now == ptrs[n - 2], "a step allocated an output"
                counts.setdefault(history, []).append(after - before)
            ptrs[n] = now
            if history:
                here = tuple(x.data_ptr() for x in t._hist if x is not None)
                assert ring is None or here == ring
                ring = here
    print("allocations per steady-state step: history=0 %s, history=5 %s" % (counts[0], counts[5]))
    assert counts[5] == counts[0]                        # the smoothing step adds no allocation to the step


def test_init_hides_the_old_slots(ahv, ops, dev, pair):
    vs, vt, w = pair
    t, outs, paths = _trajectory(ahv, dev, pair, 6, history=5)
    assert tuple(paths[-1].idx.shape) == (B, 5)
    old = [x.clone() for x in t._hist if x is not None]
    t.init(vs, vt, _t(ahv.rotations.haar_rotations_np(300, seed=6)).to(dev))
    with pytest.raises(RuntimeError, match="before the first step"):
        t.smoothed()
    for x, y in zip([x for x in t._hist if x is not None], old):
        assert _bytes_equal(x, y)                         # init does not clear the ring
    o = t.step(vs, vt)
    p = t.smoothed()
    rows = torch.arange(B, device=dev)
    assert tuple(p.idx.shape) == (B, 1) and torch.equal(o.scores[rows, p.idx[:, 0]], o.scores.max(dim=1).values)
    assert (t._hist.back[1] == -1).all()                  # frame 1 saw no predecessors, though slot 0 holds frame 5 of the old run
    full = ops.smooth_backtrace(t._hist, t.step_counter, frames=5)
    assert (full.idx[:, :4] == -1).all() and torch.equal(full.idx[:, 4], p.idx[:, 0])
    for k in range(4):
        assert _bytes_equal(full.R[:, k], torch.eye(3).expand(B, 3, 3))


# ---- 7. the planted sequence with two distractor frames, on the device ----------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_distractor_on_the_device(ahv, ops, dev, s):
    """smooth_reference.DISTRACTED with the device's noise: the filter's reported pose is more than 90 degrees off on frames 5
    and 8 (the premise), and the smoothed path's largest error over frames 4-11 stays below the blind 4 096-hypothesis median
    of the clean sequence."""
    P = sm.DISTRACTED
    h = load_golden("score_n128")
    w = tuple(_t(h[k]).to(dev) for k in ("W1", "W2", "b2"))
    vs = _t(h["vol_src"]).to(dev)
    R0 = _t(tr.planted_init(ahv.rotations, s)).to(dev)
    t = ahv.track.PoseTracker(*w, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"], temperature=P["temperature"],
                              batch=1, seed=s, history=P["history"], smooth_sigma_deg=P["smooth_sigma_deg"], smooth_jump=P["smooth_jump"])
    rotate = lambda R: ops.rotate_volume(vs, _t(R[None].astype(np.float32)).to(dev))
    filt, smooth = sm.distracted_run(ahv.rotations, s, rotate, lambda vt: t.init(vs, vt, R0), lambda vt: t.step(vs, vt), t.smoothed)
    gt = tr.planted_truth(ahv.rotations, s)
    blind = []
    for k in range(P["frames"]):
        Rb = ops.select_rotation(ops.verify_pair(vs, rotate(gt[k]), R0, *w, want_scores=False)[1], R0)[2][0].cpu().numpy()
        blind.append(float(tr.geodesic_deg(Rb.astype(np.float64), gt[k])))
    worst, median = sm.distracted_bar(smooth, blind)
    print("distractor s=%d on the device: filter %s | smoothed (frames 1-11) %s | smoothed max over 4-11 %.3f | blind median %.3f"
          % (s, " ".join("%.2f" % e for e in filt), " ".join("%.2f" % e for e in smooth), worst, median))
    for k in P["distractors"]:
        assert filt[k] > 90.0, (k, filt[k])
    assert worst < median
