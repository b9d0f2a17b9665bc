"""Pose posterior on the GPU: ``ahv_pose_posterior_f32`` / ``_merge`` / ``_finish_f32`` through ``ops.pose_posterior`` and its
companions against the numpy fp64 reference (tests/posterior_reference.py).

Inputs: Haar rotations from a seeded numpy generator, planted-peak scores around two poses per sample, anchors = the modes of
``modes_reference.select_modes`` at 30 degrees, K = 4 (``posterior_reference.make_inputs``).  Every comparison first ASSERTS
the reference's decision margin (the smallest |t - min_trace| it met, t in fp64) >= 1e-4 -- an fp32 summation order moves t by
~1e-6, so the kernel cannot assign a hypothesis differently -- and that every mode bucket is well conditioned (sigma_2 + sigma_3
>= 0.5).  The seeds were chosen on the CPU so that both hold; a failing condition means the input is wrong, never the kernel.

Tolerance: 4 x the error of the stock fp32 torch composition on the CPU (``posterior_reference.stock_fp32``: softmax, masked
sums, einsum, torch.linalg.svd) against the same fp64 reference, measured over exactly the CASES below at both temperatures:
scalars 4.8e-6, mean rotations 0.056 degrees, spreads 0.040 degrees.  (The two angles are dominated by acos near 1: an fp32
matrix is orthonormal to ~1e-7, which the trace formula turns into ~0.03 degrees.)  The kernels measured against the reference
on an MI355X over the same cases: scalars 7.2e-8, mean rotations 0.016 degrees, spreads 3.8e-6 degrees."""
import numpy as np
import pytest
import torch

from . import posterior_reference as pr
from .conftest import load_golden

pytestmark = pytest.mark.gpu

STOCK_ERR_SCALAR, STOCK_ERR_ROT_DEG, STOCK_ERR_SPREAD_DEG = 4.8e-6, 0.056, 0.040
TOL_SCALAR, TOL_ROT_DEG, TOL_SPREAD_DEG = 4 * STOCK_ERR_SCALAR, 4 * STOCK_ERR_ROT_DEG, 4 * STOCK_ERR_SPREAD_DEG
MARGIN, MIN_COND = 1e-4, 0.5
ANGLE = 30.0
# (N, B, per-sample R) -> seed; per-sample R with N = 1021 / 1025 / 4099: sample 1's rows start off the 16-byte grid
CASES = {(N, B, per): 0 for N in (1, 3, 1021, 1024, 1025, 4099) for B in (1, 3) for per in (False, True)}
CASES.update({(1021, 3, True): 1, (1025, 3, True): 2, (4099, 3, True): 1})


@pytest.fixture(scope="module")
def dev(ahv):
    return torch.device("cuda:0")


_inputs = {}


def inputs(N, B, per, K=4):
    """(scores, R, anchors) of a case, computed once and never modified."""
    key = (N, B, per, K)
    if key not in _inputs:
        _inputs[key] = pr.make_inputs(N, B, per, CASES[(N, B, per)], K=K, angle_deg=ANGLE)
    return _inputs[key]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(x, y):
    """torch.equal on the bits (a NaN spread of an empty bucket equals itself)."""
    v = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return torch.equal(v(x), v(y))


def as_np(post):
    return {k: getattr(post, k).cpu().numpy() for k in pr.FIELDS}


def check(got, want, margin, label="", need_cond=True):
    """Conditions, then the tolerances.  Prints every figure before it asserts.  ``need_cond=False``: a test whose buckets are
    wide caps on purpose; mean rotations are then compared only for the buckets that meet the conditioning bound."""
    K = want["mode_prob"].shape[1]
    cond = want["cond"]
    modes_cond = cond[:, :K][~np.isnan(cond[:, :K])]
    e = pr.errors(got, want, cond, MIN_COND)
    print("%s margin %.2e  min mode cond %.3f  errors scalar %.2e  rot %.2e deg  spread %.2e deg"
          % (label, margin, modes_cond.min() if modes_cond.size else np.inf, e["scalar"], e["rot_deg"], e["spread_deg"]))
    assert margin >= MARGIN
    assert not need_cond or np.all(modes_cond >= MIN_COND)
    assert np.array_equal(got["n_excluded"], want["n_excluded"])
    assert e["scalar"] <= TOL_SCALAR and e["rot_deg"] <= TOL_ROT_DEG and e["spread_deg"] <= TOL_SPREAD_DEG
    total = got["mode_prob"].sum(axis=1, dtype=np.float64) + got["rest_prob"]
    live = np.isfinite(want["log_z"]) & (want["log_z"] > -np.inf)
    assert np.all(np.abs(total[live] - 1.0) <= 1e-6) and np.all(got["mode_prob"] >= 0) and np.all(got["rest_prob"] >= 0)
    return e


# ---- shapes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,B,per", sorted(CASES))
def test_shapes_against_the_reference(ahv, dev, N, B, per):
    s, R, A = inputs(N, B, per)
    for temp in (0.1, 0.02):
        want, margin = pr.posterior(s, R, A, ANGLE, temp)
        post = ahv.ops.pose_posterior(T(s, dev), T(R, dev), temp, anchors=T(A, dev), min_angle_deg=ANGLE)
        check(as_np(post), want, margin, "N=%d B=%d per=%s T=%g:" % (N, B, per, temp))
        assert post.state.shape == (B, pr.state_stride(4)) and post.state.dtype == torch.uint8
    # membership counts, via the masses of a constant-score run (w = 1 for every member): exact
    const = np.full_like(s, 0.25)
    st = pr.from_bytes(ahv.ops.pose_posterior(T(const, dev), T(R, dev), 0.1, anchors=T(A, dev), min_angle_deg=ANGLE).state.cpu().numpy(), 4)
    ref_states, margin = pr.batch_states(const, R, A, ANGLE, 0.1)
    assert margin >= MARGIN
    for b in range(B):
        assert np.array_equal(st[b]["rec"][:, 1], ref_states[b]["rec"][:, 1]), (b, st[b]["rec"][:, 1], ref_states[b]["rec"][:, 1])
        assert st[b]["rec"][:5, 1].sum() == N == st[b]["rec"][5, 1] and st[b]["n_excluded"] == 0


@pytest.mark.parametrize("K", [0, 1, 4, 16])
def test_anchor_counts(ahv, dev, K):
    """K = 0 (no anchors), 1, 4, and 16 = the four modes padded with empty slots, at N = 4099 (five workgroups per sample)."""
    s, R, A4 = inputs(4099, 3, False)
    A = np.zeros((3, K, 3, 3), np.float32)
    A[:, :min(K, 4)] = A4[:, :min(K, 4)]
    for temp in (0.1, 0.02):
        want, margin = pr.posterior(s, R, A if K else None, ANGLE, temp)
        post = ahv.ops.pose_posterior(T(s, dev), T(R, dev), temp, anchors=T(A, dev) if K else None,
                                      min_angle_deg=ANGLE if K else None)
        got = as_np(post)
        check(got, want, margin if K else np.inf, "K=%d T=%g:" % (K, temp))
        assert got["mode_prob"].shape == (3, K) and got["mode_R_mean"].shape == (3, K, 3, 3)
        if K == 16:
            assert np.all(got["mode_prob"][:, 4:] == 0) and np.all(got["mode_R_mean"][:, 4:] == 0)
            assert np.all(np.isnan(got["mode_spread_deg"][:, 4:]))


# ---- the reference's loss -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["a_", "b_"])
def test_infonce_loss_of_the_golden_run(ahv, dev, case):
    """G11: one anchor = the ground truth, theta = ACC_THR, T = 0.1: -log(mode_prob[:, 0]) is the reference's per-sample loss."""
    g = load_golden("infonce_grad")
    post = ahv.ops.pose_posterior(T(g[case + "sim"], dev), T(g[case + "R"], dev), 0.1, anchors=T(g[case + "gt"][:, None], dev),
                                  min_angle_deg=float(g["acc_thr"]))
    loss = -np.log(post.mode_prob[:, 0].cpu().numpy().astype(np.float64))
    print(case, loss, g[case + "loss_per_sample"])
    assert np.all(np.abs(loss - g[case + "loss_per_sample"]) <= 1e-5)
    st = pr.from_bytes(ahv.ops.pose_posterior(T(np.zeros_like(g[case + "sim"]), dev), T(g[case + "R"], dev), 0.1,
                                              anchors=T(g[case + "gt"][:, None], dev),
                                              min_angle_deg=float(g["acc_thr"])).state.cpu().numpy(), 1)
    assert [int(x["rec"][0, 1]) for x in st] == g[case + "positive"].sum(axis=1).tolist()


# ---- non-finite scores, empty sets and slots --------------------------------------------------------------------------------

def test_non_finite_scores_are_excluded_and_counted(ahv, dev):
    s, R, A = inputs(4099, 3, False)
    s = s.copy()
    s[0, 5], s[0, 1030], s[0, 4098] = np.nan, np.inf, -np.inf
    s[1] = np.nan                                              # an empty scored set between two live samples
    want, margin = pr.posterior(s, R, A, ANGLE, 0.1)
    post = ahv.ops.pose_posterior(T(s, dev), T(R, dev), 0.1, anchors=T(A, dev), min_angle_deg=ANGLE)
    got = as_np(post)
    check(got, want, margin, "non-finite:")
    assert got["n_excluded"].tolist() == [3, 4099, 0]
    assert got["log_z"][1] == -np.inf and np.isnan(got["entropy"][1]) and np.isnan(got["mean_score"][1])
    assert np.all(got["mode_prob"][1] == 0) and got["rest_prob"][1] == 0 and np.all(got["mode_R_mean"][1] == 0)
    assert np.all(got["R_mean"][1] == 0) and np.all(np.isnan(got["mode_spread_deg"][1])) and np.isnan(got["spread_deg"][1])
    # the neighbours of the empty sample are what they are without it, bit for bit
    s0, _, _ = inputs(4099, 3, False)
    s2 = s0.copy()
    s2[0] = s[0]
    other = ahv.ops.pose_posterior(T(s2, dev), T(R, dev), 0.1, anchors=T(A, dev), min_angle_deg=ANGLE)
    for k in pr.FIELDS:
        assert same(getattr(post, k)[[0, 2]].contiguous(), getattr(other, k)[[0, 2]].contiguous()), k
    assert torch.equal(post.state[[0, 2]], other.state[[0, 2]])


def test_empty_and_nan_anchor_slots_take_no_mass(ahv, dev):
    """At 150 degrees t = 0 >= min_trace holds for a zero matrix: the empty slot is skipped by its flag.  A NaN anchor matches
    nothing (and is no empty slot)."""
    s, R, A4 = inputs(1021, 1, False)
    A = A4.copy()
    A[:, 0] = 0.0
    A[:, 2, 1, 1] = np.nan
    assert pr.tau_of(150.0) < 0
    want, margin = pr.posterior(s, R, A, 150.0, 0.1)
    got = as_np(ahv.ops.pose_posterior(T(s, dev), T(R, dev), 0.1, anchors=T(A, dev), min_angle_deg=150.0))
    check(got, want, margin, "slots:", need_cond=False)   # a 150-degree cap is most of SO(3): sigma_2 + sigma_3 = 0.41 for one
    assert got["mode_prob"][0, 0] == 0 and got["mode_prob"][0, 2] == 0 and got["mode_prob"][0, 1] > 0.5


# ---- composition ----------------------------------------------------------------------------------------------------------

def test_chunks_and_shards_compose(ahv, dev):
    s, R, A = inputs(4099, 3, True)
    want, margin = pr.posterior(s, R, A, ANGLE, 0.1)
    sd, Rd, Ad = T(s, dev), T(R, dev), T(A, dev)
    one = ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=ANGLE)
    check(as_np(one), want, margin, "single call:")
    # chunks of 1000 merged INTO the state
    state = ahv.ops.pose_posterior_state(3, 4, dev)
    for i, lo in enumerate(range(0, 4099, 1000)):
        post = ahv.ops.pose_posterior(sd[:, lo:lo + 1000].contiguous(), Rd[:, lo:lo + 1000].contiguous(), 0.1, anchors=Ad,
                                      min_angle_deg=ANGLE, state=state, reset=(i == 0))
        assert post.state.data_ptr() == state.data_ptr()
    check(as_np(post), want, margin, "chunks of 1000:")
    # three uneven shards, each a state of its own, through the merge entry point
    cuts = [0, 700, 2900, 4099]
    states = torch.stack([ahv.ops.pose_posterior(sd[:, a:b].contiguous(), Rd[:, a:b].contiguous(), 0.1, anchors=Ad,
                                                 min_angle_deg=ANGLE).state for a, b in zip(cuts, cuts[1:])])
    merged = ahv.ops.merge_posterior(states, 4, 0.1)
    check(as_np(ahv.ops.pose_posterior_finish(merged, 4, 0.1)), want, margin, "3 shards:")
    # an empty chunk changes nothing; N = 0 with reset makes an empty state
    before = state.clone()
    ahv.ops.pose_posterior(sd[:, :0].contiguous(), Rd[:, :0].contiguous(), 0.1, anchors=Ad, min_angle_deg=ANGLE, state=state)
    assert torch.equal(state, before)
    empty = ahv.ops.pose_posterior(sd[:, :0].contiguous(), Rd[:, :0].contiguous(), 0.1, anchors=Ad, min_angle_deg=ANGLE)
    assert bool((empty.log_z == -np.inf).all()) and bool((empty.mode_prob == 0).all()) and bool((empty.n_excluded == 0).all())


def test_same_call_twice_is_bit_identical(ahv, dev):
    s, R, A = inputs(4099, 3, True)
    a = ahv.ops.pose_posterior(T(s, dev), T(R, dev), 0.02, anchors=T(A, dev), min_angle_deg=ANGLE)
    b = ahv.ops.pose_posterior(T(s, dev), T(R, dev), 0.02, anchors=T(A, dev), min_angle_deg=ANGLE)
    assert torch.equal(a.state, b.state)
    for k in pr.FIELDS:
        assert same(getattr(a, k), getattr(b, k)), k


def test_graph_capture_replays_the_eager_result(ahv, dev):
    """Preallocated state and workspace, one stream, no parallel branches."""
    s, R, A = inputs(4099, 3, False)
    sd, Rd, Ad = T(s, dev), T(R, dev), T(A, dev)
    eager = ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=ANGLE)
    state = ahv.ops.pose_posterior_state(3, 4, dev)
    ws = ahv.ops.pose_posterior_workspace(3, 4099, 4, dev)
    assert ws.numel() == ahv._lib.load().ahv_pose_posterior_workspace_bytes(3, 4099, 4)
    ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=ANGLE, state=state, workspace=ws, reset=True)   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            post = ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=ANGLE, state=state, workspace=ws, reset=True)
    for _ in range(2):
        state.zero_()
        for k in pr.FIELDS:
            getattr(post, k).zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(post.state, eager.state)
        for k in pr.FIELDS:
            assert same(getattr(post, k), getattr(eager, k)), k
    with pytest.raises(RuntimeError, match="workspace"):
        ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=ANGLE, workspace=ws[:100])


# ---- the verify step ------------------------------------------------------------------------------------------------------

def test_verify_pair_posterior_is_the_op_sequence(ahv, dev, g128):
    g = load_golden("batched")
    vs, vt = T(g["vol_src"], dev), T(g["vol_tgt"], dev)
    W1, W2, b2 = (T(g128[k], dev) for k in ("W1", "W2", "b2"))
    R = T(pr.haar(np.random.default_rng(5), 1021), dev)
    K = 4
    m_s, m_i, m_R, post = ahv.ops.verify_pair_posterior(vs, vt, R, W1, W2, b2, K, ANGLE, temperature=0.1)
    ref = ahv.ops.verify_pair_modes(vs, vt, R, W1, W2, b2, K, ANGLE)
    for x, y in zip((m_s, m_i, m_R), ref):
        assert torch.equal(x, y)
    scores = ahv.ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True)[0]
    keys = ahv.ops.topk_modes(scores, R, K, ANGLE)
    step = ahv.ops.pose_posterior(scores, R, 0.1, anchors=ahv.ops.select_topk(keys, R)[2], min_angle_deg=ANGLE)
    assert torch.equal(post.state, step.state)
    for k in pr.FIELDS:
        assert same(getattr(post, k), getattr(step, k)), k
    # the first mode is the arg-max: it holds its own cap's mass, and the numbers are a distribution
    assert bool((post.mode_prob[:, 0] > 0).all())
    assert bool(((post.mode_prob.sum(dim=1) + post.rest_prob - 1).abs() <= 1e-6).all())
