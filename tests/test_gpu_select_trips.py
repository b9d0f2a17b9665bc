"""Second trips of the selection kernels' tile walk on the GPU: the loops ``for (t = blockIdx.x; t < tiles; t += gridDim.x)`` of
ahv_select.hip (modes, modes modulo a group, fold), ahv_views.hip (fuse, compact fuse) and ahv_posterior.hip (posterior, resample)
and the lane-strided loops of ``resample_scan_kernel`` and ``view_compact_kernel<true>``, at sizes where a workgroup (a lane) takes
a second and a third tile -- each kernel against its existing reference under the rule its own test file states, unchanged.

Inputs: tests/select_trip_cases.py (a Haar base set of 4099 repeated cyclically, so that the reference's decision margin is that of
an N = 4099 case; scores drawn per hypothesis); tests/test_select_trip_cases_cpu.py asserts on the CPU what is assumed of them
here (margins, conditioning, where every plant sits, the walk of every size).  Sizes: cap 63 (posterior) 64 512 (no second trip:
the control), 64 513, 129 027; 64 lanes (scan, compaction counts) 65 537, 131 075; cap 1024 (``tile_grid``) 1 048 577, 1 049 603.

1. MODES.  Plants at 1 049 603 (select_trip_cases.modes_plants): sample 0 -- (a) the row's largest score at N - 1, so the round-0
   winner lives in a second trip; (b) the next-largest at N - 1 - 4099, the same matrix: not listed.  (The second trip holds 1027
   hypotheses, fewer than a period, so (b) lies in a first-trip tile: the kill of a second-trip winner has to reach it; the kill
   INSIDE a second trip is (c)'s.)  Sample 1 -- (c) the largest score in the first trip and its copy in the last tile with the
   next-largest score: not listed; (d) a hypothesis in the last tile outside tau of both earlier winners with the score that makes
   it the third entry.  At 1 048 577 only (a) fits.
2. MODES MODULO A GROUP AND THE FOLD, d2 and the axial group, test_gpu_sym.py's rules: (b) and (c) with an orbit member (R_w S_1,
   R_w Rot(axis, 100 degrees)) in place of the copy, per-sample R and one list over a shared R; the fold with ``keep`` cutting
   inside tile 1024 and with keep = 2.
3. POSTERIOR.  test_gpu_posterior.py's ``check`` and its rule for the bars -- 4 x the error of the stock fp32 torch composition
   against fp64 over exactly the cases (select_trip_cases.POST_CASES, both temperatures), measured on the CPU (the twin measures
   it again): scalars 4.3e-7, mean rotations 0.0494 degrees, spreads 1.17e-3 degrees.  (Lower than the figures of
   test_gpu_posterior.py, which were measured over that file's own, smaller cases: its constants are not reused.)  The kernels
   measured against the reference on an MI355X over the same cases: scalars 5.5e-8, mean rotations 0.0138 degrees, spreads
   3.7e-6 degrees.
4. RESAMPLE at 65 537, 131 075 (the scan's lane-strided loops) and 1 048 577, 1 049 603 (partial and emit): equal rows bit for
   bit for M = 5000 and 2 N + 1 and every u; random rows with holes draw by draw (``check_draws``, its derived eps 1.0e-5; the
   worst CDF miss measured 6.8e-11); rows whose weight lives in the last tile; a row without a finite score; a dirty workspace.
5. MULTI-VIEW FUSE AND COMPACTION, V = 3 at 60 degrees with the middle weight 0: the dense fuse with and without the limit and the
   compact fuse (bit for bit the dense one) at the ``tile_grid`` sizes, the best key planted at N - 1; the compaction's slot map,
   counts, count-only launch and identity padding at 65 537 and 131 075.

Budget: the largest device copies are a per-sample R at 1 049 603 (75 MB), view scores (25 MB) and a draw list of 2 N + 1 int64
(17 MB per sample); every test spends its time in the CPU reference.  Measured on an MI355X host: the file's 41 tests take 17 s;
the slowest are the d2 mode list (2.1 s), the d2 and axial folds with keep = 2 (1.3 s, 1.0 s), the axial mode lists (0.9 s), the
equal rows at M = 2 N + 1 (0.8 s) and the plain mode lists (0.3 - 0.6 s); every other test is under 0.6 s.

THE CHECK THAT THESE TESTS CAN FAIL.  One deliberately wrong build, not kept: every walk above stops after its first trip (the
loop's increment replaced by ``t = tiles``; likewise the three lane-strided loops of the scan and the one of the compaction).
Skipping tiles omits in-bounds work only.  The selection tests were run once on it.  Outcome: test_gpu_modes.py, test_gpu_sym.py,
test_gpu_posterior.py, test_gpu_resample.py, test_gpu_views.py and test_gpu_views_compact.py pass in full (280 tests: none of them
reaches a second trip).  Of this file's 41 tests 40 fail, each on an assertion of its own -- group 1: all three lists; group 2:
all three symmetric lists and all four folds; group 3: 64 513 (ONE hypothesis dropped: scalar error 6.6e-6 against the bar of 1.7e-6,
which the bars of test_gpu_posterior.py would have let through, and the membership counts), both 129 027 cases (scalar error
0.086), the non-finite and the composition test; group 4: every equal-rows, random-rows and last-tile test at all four sizes;
group 5: all three dense fuses, all three compactions, all three compact fuses.  The one test that passes is the posterior at
64 512, the control: 63 full tiles, no second trip, as tests/test_select_trip_cases_cpu.py states.
"""
import numpy as np
import pytest
import torch

from . import posterior_reference as pr
from . import resample_reference as rr
from . import select_trip_cases as tc
from . import sym_reference as sr
from . import views_compact_reference as vcr
from . import views_reference as vr
from .test_gpu_sym import MARGIN as SYM_MARGIN
from .test_gpu_sym import MAX_LEFT_OUT, measure_fold, run_fold
from .test_gpu_views import check_fused
from .test_gpu_views_compact import bits

pytestmark = pytest.mark.gpu

MARGIN, MIN_COND = tc.MARGIN, tc.MIN_COND
TOL = {k: 4.0 * v for k, v in tc.POST_STOCK_ERR.items()}


@pytest.fixture(scope="module")
def dev(ahv):
    ahv._lib.load()  # raises if libahv_hip.so is missing: no fallback
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. modes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,per_sample", sorted(tc.MODES_CASES))
def test_modes_list_equals_the_reference(ahv, dev, N, per_sample):
    s, R, plants = tc.modes_case(N, per_sample)
    want, margin = tc.modes_want(N, per_sample)
    print("modes N=%d per=%s: margin %.3e" % (N, per_sample, margin))
    assert margin >= MARGIN
    sd = T(s, dev)
    got = ahv.ops.topk_modes(sd, T(R, dev), tc.MODES_K, tc.MODES_ANGLE, n_offset=tc.MODES_OFFSET).cpu()
    assert got.shape == (tc.MODES_B, tc.MODES_K) and got.dtype == torch.int64
    assert torch.equal(got, torch.from_numpy(want))
    tc.check_modes_plants(got.numpy(), plants)
    assert torch.equal(got[:, 0], ahv.ops.argmax(sd, n_offset=tc.MODES_OFFSET, return_key=True).cpu())


# ---- 2. modes modulo a group, and the fold ------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,per_sample", tc.SYM_MODES_CASES)
def test_sym_modes_list_equals_the_reference(ahv, dev, group, per_sample):
    s, R, sym, plants = tc.sym_case(group, per_sample)
    want, margin = tc.sym_want(group, per_sample)
    print("sym modes %s per=%s: margin %.3e" % (group, per_sample, margin))
    assert margin > SYM_MARGIN                                   # no case is left out
    got = ahv.ops.topk_modes(T(s, dev), T(R, dev), tc.SYM_K, tc.SYM_ANGLE, n_offset=tc.SYM_OFFSET, symmetry=sym.to(dev)).cpu()
    assert torch.equal(got, torch.from_numpy(want))
    tc.check_modes_plants(got.numpy(), plants, tc.SYM_OFFSET)
    # the plain list keeps the orbit members the symmetric one drops: they are 100 degrees or more from their winners
    plain = sr.indices(ahv.ops.topk_modes(T(s, dev), T(R, dev), tc.SYM_K, tc.SYM_ANGLE, n_offset=tc.SYM_OFFSET).cpu().numpy()) - tc.SYM_OFFSET
    assert plain[0, 1] == plants["b"][1] and plain[1, 1] == plants["c_copy"][1]


@pytest.mark.parametrize("keep", [tc.FOLD_KEEP, 2])
@pytest.mark.parametrize("group", sorted(tc.SYM_GROUPS))
def test_fold_against_the_reference(ahv, dev, group, keep):
    """test_gpu_sym.py's test_fold_against_the_reference on the trip case: which / elem / trace, R_out and V_out; in place equals
    out of place bit for bit."""
    R, sym, anchors, V = tc.fold_case(group)
    r = measure_fold(ahv, dev, R, sym, anchors, V, tc.FOLD_ANGLE, keep, False, "fold %s keep=%d" % (group, keep))
    assert r["left_out"] <= MAX_LEFT_OUT
    assert r["decisions"] and r["bytes"] and r["untaken"] and r["folded"] > 300
    for k, t, floor in zip(r["e_kern"], r["e_torch"], r["floor"]):
        assert k <= 4.0 * max(t, floor)
    a = run_fold(ahv, dev, R, sym, anchors, V, tc.FOLD_ANGLE, keep, False)
    b = run_fold(ahv, dev, R, sym, anchors, V, tc.FOLD_ANGLE, keep, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- 3. posterior -----------------------------------------------------------------------------------------------------------

def as_np(post):
    return {k: getattr(post, k).cpu().numpy() for k in pr.FIELDS}


def same(x, y):
    v = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return torch.equal(v(x), v(y))


def check(got, want, margin, label=""):
    """test_gpu_posterior.check with this file's bars: conditions, then the tolerances.  Prints every figure before it asserts."""
    K = want["mode_prob"].shape[1]
    cond = want["cond"]
    modes_cond = cond[:, :K][~np.isnan(cond[:, :K])]
    e = pr.errors(got, want, cond, MIN_COND)
    print("%s margin %.2e  min mode cond %.3f  errors scalar %.2e  rot %.2e deg  spread %.2e deg"
          % (label, margin, modes_cond.min() if modes_cond.size else np.inf, e["scalar"], e["rot_deg"], e["spread_deg"]))
    assert margin >= MARGIN
    assert np.all(modes_cond >= MIN_COND)
    assert np.array_equal(got["n_excluded"], want["n_excluded"])
    assert e["scalar"] <= TOL["scalar"] and e["rot_deg"] <= TOL["rot_deg"] and e["spread_deg"] <= TOL["spread_deg"]
    total = got["mode_prob"].sum(axis=1, dtype=np.float64) + got["rest_prob"]
    live = np.isfinite(want["log_z"]) & (want["log_z"] > -np.inf)
    assert np.all(np.abs(total[live] - 1.0) <= 1e-6) and np.all(got["mode_prob"] >= 0) and np.all(got["rest_prob"] >= 0)
    return e


def posterior(ahv, dev, s, R, A, temp, **kw):
    return ahv.ops.pose_posterior(T(s, dev), T(R, dev), temp, anchors=T(A, dev), min_angle_deg=tc.POST_ANGLE, **kw)


@pytest.mark.parametrize("N,per_sample", sorted(tc.POST_CASES))
def test_posterior_against_the_reference(ahv, dev, N, per_sample):
    s, R, A = tc.posterior_case(N, per_sample)
    B, K = tc.POST_B, tc.POST_K
    lib = ahv._lib.load()
    assert lib.ahv_pose_posterior_state_bytes(B, K) == B * pr.state_stride(K)
    assert lib.ahv_pose_posterior_workspace_bytes(B, N, K) == tc.POST_MAX_PARTS * lib.ahv_pose_posterior_state_bytes(B, K)
    for temp in tc.POST_TEMPS:
        want, margin = tc.posterior_want(N, per_sample, temp)
        post = posterior(ahv, dev, s, R, A, temp)
        check(as_np(post), want, margin, "N=%d per=%s T=%g:" % (N, per_sample, temp))
        again = posterior(ahv, dev, s, R, A, temp)              # two identical calls: the same bytes
        assert torch.equal(post.state, again.state) and all(same(getattr(post, k), getattr(again, k)) for k in pr.FIELDS)
    # membership counts, via the masses of a constant-score run (w = 1 for every member): exact
    const = np.full_like(s, 0.25)
    st = pr.from_bytes(posterior(ahv, dev, const, R, A, 0.1).state.cpu().numpy(), K)
    ref_states, margin = pr.batch_states(const, R, A, tc.POST_ANGLE, 0.1)
    assert margin >= MARGIN
    for b in range(B):
        assert np.array_equal(st[b]["rec"][:, 1], ref_states[b]["rec"][:, 1]), (b, st[b]["rec"][:, 1], ref_states[b]["rec"][:, 1])
        assert st[b]["rec"][:K + 1, 1].sum() == N == st[b]["rec"][K + 1, 1] and st[b]["n_excluded"] == 0


def test_posterior_non_finite_scores_in_every_trip(ahv, dev):
    """NaN, +inf and -inf in first-, second- and third-trip tiles (select_trip_cases.POST_HOLES) are excluded and counted; a
    sample of all-NaN scores between two live ones leaves its neighbours' states as they are without it, bit for bit."""
    N = 129027
    s0, R, A = tc.posterior_case(N, True)
    s = s0.copy()
    for b, t, place, value in tc.POST_HOLES:
        s[b, t * tc.TILE + place] = value
    s[1] = np.nan
    want, margin = pr.posterior(s, R, A, tc.POST_ANGLE, 0.1)
    post = posterior(ahv, dev, s, R, A, 0.1)
    got = as_np(post)
    check(got, want, margin, "non-finite:")
    assert got["n_excluded"].tolist() == [4, N, 3]
    assert got["log_z"][1] == -np.inf and np.all(got["mode_prob"][1] == 0) and got["rest_prob"][1] == 0
    s2 = s0.copy()
    s2[0], s2[2] = s[0], s[2]
    other = posterior(ahv, dev, s2, R, A, 0.1)
    for k in pr.FIELDS:
        assert same(getattr(post, k)[[0, 2]].contiguous(), getattr(other, k)[[0, 2]].contiguous()), k
    assert torch.equal(post.state[[0, 2]], other.state[[0, 2]])


def test_posterior_chunks_of_one_trip_compose(ahv, dev):
    """One call over 129 027 (three trips) against chunks of 64 512 (one trip each) merged into the state."""
    N = 129027
    s, R, A = tc.posterior_case(N, True)
    want, margin = tc.posterior_want(N, True, 0.1)
    sd, Rd, Ad = T(s, dev), T(R, dev), T(A, dev)
    one = ahv.ops.pose_posterior(sd, Rd, 0.1, anchors=Ad, min_angle_deg=tc.POST_ANGLE)
    check(as_np(one), want, margin, "single call:")
    state = ahv.ops.pose_posterior_state(tc.POST_B, tc.POST_K, dev)
    for i, lo in enumerate(range(0, N, 64512)):
        post = ahv.ops.pose_posterior(sd[:, lo:lo + 64512].contiguous(), Rd[:, lo:lo + 64512].contiguous(), 0.1, anchors=Ad,
                                      min_angle_deg=tc.POST_ANGLE, state=state, reset=(i == 0))
    assert i == 2
    check(as_np(post), want, margin, "chunks of 64 512:")


# ---- 4. resample --------------------------------------------------------------------------------------------------------------

def _u(u, dev):
    return torch.full((tc.RES_B,), u, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("big_m", [False, True])
@pytest.mark.parametrize("N", tc.RES_SIZES)
def test_resample_equal_rows_bit_for_bit(ahv, dev, N, big_m):
    """Weights of exactly 1: the draw list is the exact-arithmetic one, for M = 5000 and M = 2 N + 1 and every u."""
    s = tc.resample_equal_rows(N)
    sd = T(s, dev)
    M = 2 * N + 1 if big_m else 5000
    for temp in ((0.1,) if big_m else (0.1, 0.02)):
        for u in tc.RES_US:
            got = ahv.ops.resample(sd, M, temp, u=_u(u, dev))
            assert torch.equal(got.cpu(), torch.from_numpy(rr.resample(s, M, temp, u))), (N, M, temp, u)


@pytest.mark.parametrize("N", tc.RES_SIZES)
def test_resample_random_rows_every_draw(ahv, dev, N):
    s = tc.resample_random_rows(N)
    sd = T(s, dev)
    worst = {"eps": 0.0, "cdf_miss": 0.0, "count_miss": 0.0}
    for M, temp, us in ((5000, 0.1, tc.RES_US), (5000, 0.02, (0.0, 0.5)), (2 * N + 1, 0.1, (0.0, 0.5))):
        beta = rr.beta_of(temp)
        for u in us:
            got = ahv.ops.resample(sd, M, temp, u=_u(u, dev)).cpu().numpy()
            assert got.shape == (tc.RES_B, M) and got.dtype == np.int64
            for b in range(tc.RES_B):
                fig = rr.check_draws(got[b], s[b], beta, u)         # exact invariants, then every draw to its derived eps
                worst = {k: max(worst[k], fig[k]) for k in worst}
    print("N=%d: eps %.3e, worst CDF miss %.3e, worst |count - M p| %.4f" % (N, worst["eps"], worst["cdf_miss"], worst["count_miss"]))


@pytest.mark.parametrize("N", tc.RES_SIZES)
def test_resample_rows_that_live_in_the_last_tile(ahv, dev, N):
    B, M = tc.RES_B, 5000
    lib = ahv._lib.load()
    assert lib.ahv_resample_workspace_bytes(B, N) == B * (32 + 16 * (tc.tiles_of(N) + 1))     # a header and tiles + 1 records
    # a peaked row whose maximum sits in the last tile owns all M slots (exp(-1.8 / 0.02) = 8e-40 per rival)
    s = np.full((B, N), -0.9, np.float32)
    at = [N - 1, N - 2]
    for b in range(B):
        s[b, at[b]] = 0.9
    got = ahv.ops.resample(T(s, dev), M, 0.02).cpu()
    assert torch.equal(got, torch.tensor(at)[:, None].expand(B, M))
    # weight in the last tile only: the scan's last_tile is the last record, beyond record 64
    s = tc.resample_last_tile_rows(N)
    for u in (0.0, 0.5):
        got = ahv.ops.resample(T(s, dev), M, 0.1, u=_u(u, dev)).cpu()
        assert torch.equal(got, torch.from_numpy(rr.resample(s, M, 0.1, u))) and int(got.min()) >= (tc.tiles_of(N) - 1) * tc.TILE
    # a row without a finite score gives -1 everywhere; the finite row next to it is untouched by it
    s = np.full((B, N), np.nan, np.float32)
    s[0, ::2], s[0, 1::2] = np.inf, -np.inf
    s[1] = 0.5
    got = ahv.ops.resample(T(s, dev), M, 0.1).cpu()
    assert bool((got[0] == -1).all()) and torch.equal(got[1], torch.from_numpy(rr.resample(s[1:], M, 0.1))[0])
    # a garbage-filled workspace gives the same bytes
    sd = T(tc.resample_random_rows(N), dev)
    u = torch.tensor([0.1, 0.9], device=dev)
    a = ahv.ops.resample(sd, M, 0.02, u=u).clone()
    ws = ahv.ops.resample_workspace(B, N, dev)
    ws.fill_(0xFF)
    assert torch.equal(a, ahv.ops.resample(sd, M, 0.02, u=u, workspace=ws))


# ---- 5. views -------------------------------------------------------------------------------------------------------------
VIEWS_FUSE_CASES = [(1048577, True), (1049603, True), (1049603, False)]
VIEWS_COMPACT_CASES = [(65537, True), (131075, True), (131075, False)]


@pytest.mark.parametrize("N,per_sample", VIEWS_FUSE_CASES)
def test_fuse_against_the_reference(ahv, dev, N, per_sample):
    """test_gpu_views.py's acceptance of the fused row, with and without the limit; the best key is planted in a second trip."""
    ops = ahv.ops
    s, Q, A = tc.views_case(N, per_sample)
    sg, Qg, Ag = T(s, dev), T(Q, dev), T(A, dev)
    w, V, off = tc.VIEWS_WEIGHTS, tc.VIEWS_V, tc.VIEWS_OFFSET
    for theta in (None, tc.VIEWS_THETA):
        want, scale, g, margin = vr.fuse(s, Q, A, w, theta)
        assert margin >= MARGIN
        fused, key = ops.fuse_view_scores(sg, Qg, Ag, w, theta, n_offset=off)
        label = "N=%d per=%s theta=%s" % (N, per_sample, theta)
        check_fused(fused.cpu().numpy(), want, scale, V, label)
        assert torch.equal(key, ops.argmax(fused, off, return_key=True)), label
        score, idx = ops.unpack_best(key)
        assert idx.cpu().tolist() == [N - 1 + off] * tc.VIEWS_B and score.cpu().tolist() == [tc.VIEWS_BEST] * tc.VIEWS_B
        if theta is not None:
            assert 0 < g.sum() < g.size
        _, key_only = ops.fuse_view_scores(sg, Qg, Ag, w, theta, n_offset=off, want_scores=False)
        assert torch.equal(key_only, key), label


@pytest.mark.parametrize("N,per_sample", VIEWS_COMPACT_CASES)
def test_compaction_against_the_reference(ahv, dev, N, per_sample):
    """Slot map and counts exact; the count-only launch (it sizes M) agrees with the full run; the identity padding is there."""
    ops = ahv.ops
    _, Q, A = tc.views_case(N, per_sample)
    slot, counts, g, margin = tc.views_compact_want(N, per_sample)
    assert margin >= MARGIN
    Qg, Ag = T(Q, dev), T(A, dev)
    w, B, V = tc.VIEWS_WEIGHTS, tc.VIEWS_B, tc.VIEWS_V
    R, slot_g, counts_g = ops.view_rotations_compact(Qg, Ag, tc.VIEWS_THETA, w)
    M = int(counts.max())
    assert R.shape == (B, V, M, 3, 3)                              # M came from the count-only launch
    assert np.array_equal(counts_g.cpu().numpy(), counts) and np.array_equal(slot_g.cpu().numpy(), slot)
    dense = ops.view_rotations(Qg, Ag).cpu().numpy()
    assert np.array_equal(bits(R.cpu().numpy()), bits(vcr.gather(dense, slot, M)))
    eye = torch.eye(3, device=dev)
    assert torch.equal(R[:, 1], eye.expand(B, M, 3, 3))            # the absent view: identities only
    for b in range(B):
        for v in (0, 2):
            assert torch.equal(R[b, v, int(counts[b, v]):], eye.expand(M - int(counts[b, v]), 3, 3))
    cap = M + 5                                                    # a caller's capacity: no count-only launch
    R2, slot2, counts2 = ops.view_rotations_compact(Qg, Ag, tc.VIEWS_THETA, w, capacity=cap)
    assert torch.equal(slot2, slot_g) and torch.equal(counts2, counts_g)
    assert np.array_equal(bits(R2.cpu().numpy()), bits(vcr.gather(dense, slot, cap)))


@pytest.mark.parametrize("N,per_sample", VIEWS_FUSE_CASES)
def test_compact_fuse_equals_the_dense_fuse(ahv, dev, N, per_sample):
    """Random compact scores laid out by the REFERENCE's slot map (no scorer launch at these sizes): the compact fuse gives the
    dense fuse's row and key bit for bit; the best key is planted in a second trip."""
    ops = ahv.ops
    _, Q, A = tc.views_case(N, per_sample)
    slot, counts, g, margin = tc.views_compact_want(N, per_sample)
    assert margin >= MARGIN
    w, B, V, off = tc.VIEWS_WEIGHTS, tc.VIEWS_B, tc.VIEWS_V, tc.VIEWS_OFFSET
    M = int(counts.max())
    cs = np.random.default_rng(7 * N + V + B).standard_normal((B, V, M)).astype(np.float32)
    cs[np.arange(M)[None, None] >= counts[:, :, None]] = np.nan     # past a list's end: never read
    for b in range(B):
        for v in (0, 2):
            if slot[b, v, N - 1] >= 0:
                cs[b, v, slot[b, v, N - 1]] = tc.VIEWS_BEST
    sd = vcr.scatter(cs, slot, np.nan)                               # dense layout, every other pair poisoned
    fd, kd = ops.fuse_view_scores(T(sd, dev), T(Q, dev), T(A, dev), w, tc.VIEWS_THETA, n_offset=off)
    slot_g = T(slot, dev)
    fc, kc = ops.fuse_view_scores_compact(T(cs, dev), slot_g, w, n_offset=off)
    assert torch.equal(bits(fc), bits(fd)) and torch.equal(kc, kd)
    want, scale, g2, _ = vr.fuse(sd, Q, A, w, tc.VIEWS_THETA)
    assert np.array_equal(g2, slot >= 0)
    check_fused(fc.cpu().numpy(), want, scale, V, "compact N=%d per=%s" % (N, per_sample))
    assert ops.unpack_best(kc)[1].cpu().tolist() == [N - 1 + off] * B
    none, k_only = ops.fuse_view_scores_compact(T(cs, dev), slot_g, w, n_offset=off, want_scores=False)
    assert none is None and torch.equal(k_only, kc)
