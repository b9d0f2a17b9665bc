"""Posterior resampling on the GPU: ``ops.resample`` (``ahv_resample_f32``) against the numpy reference
(tests/resample_reference.py) -- bit for bit where the weights are exactly 1, draw by draw to the derived tolerance on random
rows --, ``ops.compose_rotations_indexed``, ``ops.verify_pair_resampled`` and ``CoarseToFine(resample=True)``.

Shapes: N in {1, 3, 1021, 1024, 1025, 4099} (one hypothesis, less than a lane's four, one short of a tile, a tile, one over, four
tiles and a ragged end), B = 3 (rows with N % 4 != 0 start mid-vector), M in {1, 64, 1000, 5000} (the last exceeds every N), u in
{0, 0.5, the largest float below 1, 1.5, NaN} (the last two count as 0.5)."""
import numpy as np
import pytest
import torch

from . import resample_reference as rr
from .conftest import load_golden

pytestmark = pytest.mark.gpu

NS = [1, 3, 1021, 1024, 1025, 4099]
MS = [1, 64, 1000, 5000]
US = [0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), 1.5, float("nan")]
B = 3


@pytest.fixture(scope="module")
def dev(ahv):
    return torch.device("cuda:0")


def _u(u, dev):
    return torch.full((B,), u, dtype=torch.float32, device=dev)


def _holes(s):
    """NaN / +inf / -inf holes in rows of at least 3 scores (a different place in every row), never the whole row."""
    N = s.shape[1]
    if N >= 3:
        for b in range(s.shape[0]):
            s[b, (b + 1) % N], s[b, (N // 2 + b) % N], s[b, N - 1 - b % 2] = np.nan, np.inf, -np.inf
    return s


# ---- exact cases: weights of exactly 1 --------------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
def test_equal_rows_match_the_reference_bit_for_bit(ahv, dev, N):
    for holes in (False, True):
        s = np.full((B, N), 0.25, np.float32)
        s[1], s[2] = -0.75, 0.0
        if holes:
            s = _holes(s)
        sd = torch.from_numpy(s).to(dev)
        for M in MS:
            for T in (0.1, 0.02):
                for u in US:
                    got = ahv.ops.resample(sd, M, T, u=_u(u, dev))
                    want = torch.from_numpy(rr.resample(s, M, T, u))
                    assert torch.equal(got.cpu(), want), (N, holes, M, T, u)
                got = ahv.ops.resample(sd, M, T)                      # no u: 0.5
                assert torch.equal(got.cpu(), torch.from_numpy(rr.resample(s, M, T, 0.5))), (N, holes, M, T)


# ---- random rows: every draw ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [0.1, 0.02])
@pytest.mark.parametrize("N", NS)
def test_random_rows_every_draw(ahv, dev, N, T):
    rng = np.random.default_rng(1000 + N)
    s = _holes(rng.uniform(-0.2, 0.6, (B, N)).astype(np.float32))
    sd = torch.from_numpy(s).to(dev)
    beta = rr.beta_of(T)
    worst = {"eps": 0.0, "cdf_miss": 0.0, "count_miss": 0.0}
    for M in MS:
        for u in US:
            got = ahv.ops.resample(sd, M, T, u=_u(u, dev)).cpu().numpy()
            assert got.shape == (B, M) and got.dtype == np.int64            # every slot j in [0, M) is there once
            for b in range(B):
                fig = rr.check_draws(got[b], s[b], beta, u)                 # exact invariants, then every draw to eps
                worst = {k: max(worst[k], fig[k]) for k in worst}
    print("N=%d T=%g: eps %.3e, worst CDF miss %.3e, worst |count - M p| %.4f" % (N, T, worst["eps"], worst["cdf_miss"],
                                                                                   worst["count_miss"]))


def test_offsets_per_sample(ahv, dev):
    """u is read per sample: three different offsets in one call."""
    rng = np.random.default_rng(5)
    s = rng.uniform(-0.2, 0.6, (B, 1025)).astype(np.float32)
    u = np.array([0.0, 0.9, np.nan], np.float32)
    got = ahv.ops.resample(torch.from_numpy(s).to(dev), 1000, 0.1, u=torch.from_numpy(u).to(dev)).cpu().numpy()
    for b in range(B):
        rr.check_draws(got[b], s[b], rr.beta_of(0.1), u[b])
    assert not np.array_equal(got[0], ahv.ops.resample(torch.from_numpy(s).to(dev), 1000, 0.1).cpu().numpy()[0])


# ---- further cases ------------------------------------------------------------------------------------------------------

def test_peaked_row_goes_to_one_hypothesis(ahv, dev):
    """The balanced-emit case: one hypothesis owns all M slots (exp(-1.8 / 0.02) = 8e-40 per rival, 4098 of them)."""
    s = np.full((B, 4099), -0.9, np.float32)
    at = [0, 2048, 4098]
    for b in range(B):
        s[b, at[b]] = 0.9
    got = ahv.ops.resample(torch.from_numpy(s).to(dev), 5000, 0.02).cpu()
    assert torch.equal(got, torch.tensor(at)[:, None].expand(B, 5000))


def test_rows_without_a_finite_score(ahv, dev):
    s = np.full((B, 1025), np.nan, np.float32)
    s[1, ::2], s[1, 1::2] = np.inf, -np.inf
    s[2] = 0.5                                                  # a finite row next to them is untouched by it
    got = ahv.ops.resample(torch.from_numpy(s).to(dev), 1000, 0.1).cpu()
    assert bool((got[:2] == -1).all()) and torch.equal(got[2], torch.from_numpy(rr.resample(s[2:], 1000, 0.1))[0])


def test_two_runs_are_byte_identical(ahv, dev):
    rng = np.random.default_rng(9)
    s = torch.from_numpy(_holes(rng.uniform(-0.2, 0.6, (B, 4099)).astype(np.float32))).to(dev)
    u = torch.tensor([0.1, 0.5, 0.9], device=dev)
    a = ahv.ops.resample(s, 5000, 0.02, u=u).clone()
    ws = ahv.ops.resample_workspace(B, 4099, dev)
    ws.fill_(0xFF)                                              # a workspace of its own, with garbage in it
    b = ahv.ops.resample(s, 5000, 0.02, u=u, workspace=ws)
    assert torch.equal(a, b)


def test_graph_replay_follows_u(ahv, dev):
    rng = np.random.default_rng(13)
    s = torch.from_numpy(rng.uniform(-0.2, 0.6, (B, 4099)).astype(np.float32)).to(dev)
    M, T = 1000, 0.1
    u = torch.full((B,), 0.5, device=dev)
    out = torch.empty((B, M), dtype=torch.int64, device=dev)
    ws = ahv.ops.resample_workspace(B, 4099, dev)
    eager = {v: ahv.ops.resample(s, M, T, u=torch.full((B,), v, device=dev)).clone() for v in (0.5, 0.0)}
    assert not torch.equal(eager[0.5], eager[0.0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ahv.ops.resample(s, M, T, u=u, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ahv.ops.resample(s, M, T, u=u, out=out, workspace=ws)
    out.fill_(-7)
    graph.replay()
    assert torch.equal(out, eager[0.5])
    u.fill_(0.0)                                                # changed in place between replays: the draws follow
    graph.replay()
    assert torch.equal(out, eager[0.0])


@pytest.mark.parametrize("per_sample", [False, True])
def test_compose_rotations_indexed(ahv, dev, per_sample):
    rng = np.random.default_rng(17)
    N, M = 1021, 1000
    R = ahv.rotations.haar_rotations_np(B * N if per_sample else N, 3).reshape((B, N, 3, 3) if per_sample else (N, 3, 3))
    D = ahv.rotations.haar_rotations_np(M, 4)
    idx = rng.integers(0, N, (B, M)).astype(np.int64)
    idx[0, 5], idx[1, 0], idx[2, M - 1], idx[2, 7] = -1, N, N + 12345, -(1 << 40)      # out of range: row 0
    got = ahv.ops.compose_rotations_indexed(torch.from_numpy(idx).to(dev), torch.from_numpy(R).to(dev),
                                            torch.from_numpy(D).to(dev)).cpu().numpy()
    loc = np.where((idx < 0) | (idx >= N), 0, idx)
    seeds = R[np.arange(B)[:, None], loc] if per_sample else R[loc]
    want = np.matmul(seeds.astype(np.float64), D.astype(np.float64)[None])
    assert got.shape == (B, M, 3, 3)
    assert np.abs(got - want).max() <= 5 * 2.0 ** -24           # three products and two adds on entries <= 1


def test_verify_pair_resampled(ahv, dev, g128):
    T_ = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k])).to(dev)
    vs, vt, R, W1, W2, b2 = (T_(k) for k in ("vol_src", "vol_tgt", "R", "W1", "W2", "b2"))
    D = ahv.rotations.refine_rotations(torch.eye(3), 200, 10.0, generator=torch.Generator().manual_seed(0)).to(dev)
    u = torch.full((vs.shape[0],), 0.25, device=dev)
    r = ahv.ops.verify_pair_resampled(vs, vt, R, D, W1, W2, b2, temperature=0.05, u=u)
    s1, key1, f_tgt = ahv.ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True, want_feat_tgt=True)
    assert torch.equal(r.coarse_scores, s1) and torch.equal(r.coarse_key, key1)
    assert torch.equal(r.draws, ahv.ops.resample(s1, 200, 0.05, u=u))
    rr.check_draws(r.draws[0].cpu().numpy(), s1[0].cpu().numpy(), rr.beta_of(0.05), 0.25)
    assert torch.equal(r.R_fine, ahv.ops.compose_rotations_indexed(r.draws, R, D))
    s2 = ahv.ops.score_hypotheses(vs, f_tgt, r.R_fine, W1, W2, b2, want_scores=True)[0]
    assert torch.equal(r.fine_scores, s2)                       # its fine scores: score_hypotheses on the composed set
    best = torch.max(s2, dim=1)
    assert torch.equal(r.score, best.values) and torch.equal(r.idx, best.indices)
    assert torch.equal(r.R_pred, r.R_fine[torch.arange(len(s2), device=dev), best.indices])


def test_resampled_step_eager_equals_captured(ahv, dev, g128):
    """CoarseToFine(resample=True) at 1 024 + 256 hypotheses: the step's own checks, eager = captured, and resample=False is the
    seeds=1 step."""
    T_ = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k])).to(dev)
    g = load_golden("batched")
    vs, vt = torch.from_numpy(g["vol_src"]).to(dev), torch.from_numpy(g["vol_tgt"]).to(dev)
    W1, W2, b2 = T_("W1"), T_("W2"), T_("b2")
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(1024, 43)).to(dev)
    N2, TEMP = 256, 0.05
    u = torch.tensor([0.0, 0.5, 0.75], device=dev)
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N2, max_angle_deg=10.0, batch=B, want_scores=True, **kw)
    eager = mk(resample=True, resample_temperature=TEMP, resample_u=u, use_graph=False)
    graph = mk(resample=True, resample_temperature=TEMP, resample_u=u, use_graph=True)
    assert graph.use_graph and not eager.use_graph
    out = [t.clone() for t in eager(vs, vt)]
    score, idx, R_pred, c_score, c_idx = out
    s1, s2, draws = eager.last["coarse_scores"], eager.last["fine_scores"], eager.last["resample"].clone()
    assert draws.shape == (B, N2) and torch.equal(draws[:, 0], c_idx)
    cm = torch.max(s1, dim=1)
    assert torch.equal(c_score, cm.values) and torch.equal(c_idx, cm.indices)
    want = ahv.ops.resample(s1, N2, TEMP, u=u)
    assert torch.equal(draws[:, 1:], want[:, 1:])
    for b in range(B):
        rr.check_draws(want[b].cpu().numpy(), s1[b].cpu().numpy(), rr.beta_of(TEMP), float(u[b]))
    assert torch.equal(eager.last["R_fine"], ahv.ops.compose_rotations_indexed(draws, R, eager.D))
    fm = torch.max(s2, dim=1)
    assert torch.equal(score, fm.values) and torch.equal(idx, fm.indices) and bool(((0 <= idx) & (idx < N2)).all())
    assert torch.equal(R_pred, eager.last["R_fine"][torch.arange(B, device=dev), idx])
    assert bool((score >= c_score).all())                      # D[0] = I and slot 0 is the arg-max
    for rnd in range(2):                                        # the second round replays the captured graph
        for x, y in zip(graph(vs, vt), out):
            assert torch.equal(x, y), rnd
        assert torch.equal(graph.last["resample"], draws)
    # the regression guard: resample=False leaves the seeds=1 step as it is
    a, b_ = mk(use_graph=False), mk(resample=False, resample_temperature=0.5, resample_u=0.9, use_graph=False)
    for x, y in zip(a(vs, vt), b_(vs, vt)):
        assert torch.equal(x, y)
    assert torch.equal(a.last["fine_scores"], b_.last["fine_scores"])
    # polishing composes unchanged: never below the fine winner
    pol = mk(resample=True, resample_temperature=TEMP, resample_u=u, use_graph=False, polish_iters=2)
    p_score = pol(vs, vt)[0]
    assert bool((p_score >= score).all()) and torch.equal(pol.last["polish"]["score_before"], score)
