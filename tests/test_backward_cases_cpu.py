"""The conditions the cases of tests/backward_cases.py must meet for tests/test_gpu_backward_edges.py to mean what it says,
checked on the CPU references alone (sized for the MI355X's 256 CUs).  Nothing here measures a kernel."""
import pytest
import torch

from . import backward_cases as bc

CU = bc.CU_MI355X
S1, S2, S3 = bc.sizes(CU, 1), bc.sizes(CU, 2), bc.sizes(CU, 3)
B_MANY, N_MANY = bc.many_samples(CU)
CASES = bc.all_cases(CU)
ids = lambda c: "-".join(map(str, c))
KERNELS = ("head", "saved", "w1", "vol", "du")


def test_the_constants_are_the_headers():
    """A changed kBwd*PerWg must fail here, not hollow out the sizes."""
    assert bc.source_constants() == bc.PER_WG == {"head": 4, "saved": 8, "w1": 4, "vol": 2, "du": 1}


def test_grid_reproduces_the_table():
    names = ("one", "partial", "du_turn", "vol_turn", "head_turn", "all_exact", "all_ragged")
    assert [S3[k] for k in names] == [1, 7, 86, 171, 341, 680, 681]
    assert [S1[k] for k in names] == [1, 7, 257, 513, 1025, 2048, 2049]
    assert S2["vol_turn"] == 257 and (B_MANY, N_MANY) == (257, (1, 9))
    # gx of backward_grid for the five kernels (head, saved, w1, vol, du), B = 3: gy = 3, G = 85
    gx = {"one": (1, 1, 1, 1, 1), "partial": (2, 1, 2, 4, 7), "du_turn": (22, 11, 22, 43, 85), "vol_turn": (43, 22, 43, 85, 85),
          "head_turn": (85, 43, 85, 85, 85), "all_exact": (85,) * 5, "all_ragged": (85,) * 5}
    # (turns, hypotheses in the last turn) of each kernel's walk: WALK hypotheses per workgroup and turn (du: kernel 1's four waves)
    assert bc.WALK == {"head": 4, "saved": 8, "w1": 4, "vol": 2, "du": 4}
    walk = {"one": ((1, 1),) * 5, "partial": ((1, 7),) * 5,
            "du_turn": ((1, 86),) * 5,
            "vol_turn": ((1, 171), (1, 171), (1, 171), (2, 1), (1, 171)),
            "head_turn": ((2, 1), (1, 341), (2, 1), (3, 1), (2, 1)),
            "all_exact": ((2, 340), (1, 680), (2, 340), (4, 170), (2, 340)),
            "all_ragged": ((3, 1), (2, 1), (3, 1), (5, 1), (3, 1))}
    for k in names:
        assert tuple(bc.grid(CU, 3, S3[k], bc.PER_WG[p]) for p in KERNELS) == tuple((x, 3) for x in gx[k]), k
        assert tuple(bc.turns(CU, 3, S3[k], p) for p in KERNELS) == walk[k], k
    # B = 1: G = cu, one row of workgroups
    assert [bc.grid(CU, 1, S1["partial"], bc.PER_WG[p]) for p in KERNELS] == [(2, 1), (1, 1), (2, 1), (4, 1), (7, 1)]
    assert [bc.turns(CU, 1, S1["head_turn"], p) for p in KERNELS] == [(2, 1), (1, 1025), (2, 1), (3, 1), (2, 1)]
    assert [bc.turns(CU, 1, S1["all_ragged"], p) for p in KERNELS] == [(3, 1), (2, 1), (3, 1), (5, 1), (3, 1)]
    # B = cu + 1: gx = 1, gy = cu; row 0 takes samples 0 and cu
    for n in N_MANY:
        assert [bc.grid(CU, B_MANY, n, bc.PER_WG[p]) for p in KERNELS] == [(1, CU)] * 5
    assert [bc.turns(CU, B_MANY, 9, p) for p in KERNELS] == [(3, 1), (2, 1), (3, 1), (5, 1), (3, 1)]
    # the rotation gradient's own kernel: (gx, turns, last turn) at the sizes its cases use
    assert [bc.rotgrad_walk(CU, 3, S3[k]) for k in ("partial", "du_turn", "head_turn")] == [(7, 1, 7), (86, 1, 86), (171, 2, 170)]
    # B > cu and B < cu with a remainder; an odd CU count: sizes() checks every name with grid / turns
    assert bc.grid(CU, 300, 2, 4) == (1, CU) and bc.grid(CU, 5, 2048, 4) == (51, 5) and bc.grid(CU, 1, 0 + 1, 8) == (1, 1)
    for B in (1, 2, 3):
        s = bc.sizes(250, B)
        assert s["all_ragged"] == 8 * (250 // B) + 1
    bc.many_samples(250)
    # the size limit: the reference cost of the existing (2, 1100) case -- 3 x 681 on the grid sweep, 257 x 9 with many samples
    assert sorted(B * N for _, B, N, _ in CASES)[-4:] == [3 * 681, 1 * 2049, 257 * 9, 257 * 9] and 257 * 9 < 1.06 * 2 * 1100


def test_the_listed_cases():
    assert len(CASES) == len(set(CASES)) == 25
    kinds = {k for k, _, _, _ in CASES}
    assert kinds == set(bc.KINDS)
    assert ("plain", B_MANY, 9, False) in CASES and ("clamp", B_MANY, 9, False) in CASES and ("clamp", 2, 257, False) in CASES
    for kind, key in bc.ROTGRAD:
        assert (kind, 3, S3[key], True) in CASES


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_every_case_has_finite_references_and_a_yardstick(c):
    case = bc.backward_case(*c)
    print("%-46s e_ref %s  per-sample %.1e  u rms %.2e  near-kink %d  seed steps %d" % (
        case.name, " ".join("%.2e" % e for e in case.e_ref), case.e_ref_per_sample, case.u_rms, len(case.ref.amb), case.seed_steps))
    assert bc.conditions(case) == []
    assert (case.B, case.N) == (c[1], c[2]) and case.R.dim() == (4 if c[3] else 3)
    shapes = [(case.B, 16, 8, 8, 8), (case.B, 32, 64), (32, 384), (32, 32), (32,)]
    for g64, g32, shape in zip(case.ref.base, case.g32, shapes):
        assert tuple(g64.shape) == tuple(g32.shape) == shape and g64.dtype == torch.float64 and g32.dtype == torch.float32
        assert torch.isfinite(g64).all() and torch.isfinite(g32).all()
    # un-normalised target features, independent per sample; N(0,1) upstream gradients
    assert (case.ft.norm(dim=1) - 1).abs().min() > 1e-3 and 3 < case.ft.norm(dim=1).mean() < 8
    if case.B > 1:
        assert not torch.equal(case.ft[0], case.ft[1]) and not torch.equal(case.vs[0], case.vs[1])
    if case.kind in ("no_bias", "clamp"):
        assert not case.hd[2].any()
    # ambiguous sub-gradients: KINK_TAU at the scale of the case's own pre-activations
    assert case.scale == case.u_rms / 0.5 and case.ref.scale == case.scale
    assert len(case.ref.amb) <= bc.KINK_MAX
    for b, idx in case.ref.amb:
        assert 0 < abs(float(case.ref.us[b][tuple(idx)])) < bc.KINK_TAU * case.scale
    # the yardstick: positive wherever the gradient is not identically zero, and the bar never looser than GRAD_RTOL
    bars, bar_ps = case.bars()
    for name, g64, e, bar in zip(bc.GRAD_NAMES, case.ref.base, case.e_ref, bars):
        if g64.abs().max() > 0:
            assert e > 0, name
        else:
            assert e == 0 and bar == 0, name                 # dead_relu: d vol_src, d W1, d W2
        assert bar == min(bc.GRAD_RTOL, bc.PARITY_FACTOR * e) <= bc.GRAD_RTOL, (name, e)
    assert bar_ps <= bc.GRAD_RTOL and case.e_ref_per_sample >= case.e_ref[0] * (1 - 1e-12)
    # the fp32 reference passes its own rule (accept_grads asserts it)
    ratios = bc.accept_grads(case.g32, case, case.name + ", fp32 CPU autograd")
    assert len(ratios) == 6 and all(r <= bc.PARITY_FACTOR for r in ratios)


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == "clamp"], ids=ids)
def test_clamp_cases_keep_their_distance_from_the_clamp(c):
    case = bc.backward_case(*c)
    n64, n32 = case.norm64, case.norm32
    assert n64.shape == n32.shape == (case.B, case.N, 64) and n64.dtype == torch.float64 and n32.dtype == torch.float32
    # the norms are the reference's: its forward at this scale is v / max(|v|, EPS), so |f| = min(|v| / EPS, 1)
    f = torch.stack([bc.fc.ref64("forward_3d2d", bc.fc.ref64("rotate_volume", case.vs[b:b + 1], case.rotations(b)), *case.hd).norm(dim=1)
                     for b in range(case.B)])
    assert (f - (n64 / bc.EPS).clamp_max(1.0)).abs().max() < 1e-9
    gap = (n64 / bc.EPS - 1).abs().min().item()
    share = case.clamped().double().mean(dim=(1, 2))
    per_hyp = case.clamped().double().mean(dim=2)
    both = ((per_hyp > 0) & (per_hyp < 1)).double().mean().item()
    print("%-46s nearest norm %.2e of EPS away; clamped %.3f .. %.3f per sample; both sides in %.3f of the hypotheses" % (
        case.name, gap, share.min(), share.max(), both))
    assert gap >= bc.CLAMP_GAP                                          # (a)
    assert (share >= 0.4).all() and (share <= 0.6).all()                # (b)
    assert both >= 0.9                                                  # (c)
    assert torch.equal(n32 < bc.EPS, n64 < bc.EPS)                      # (d)
    assert ((n32.double() / n64 - 1).abs().max() < gap / 4)             # ... with room: fp32's norms are far nearer to fp64's than to EPS
    # squares stay clear of the fp32 denormal range, and the magnitudes stay inside fp32
    assert n64.min() > 1e-14 and case.vs.abs().max() < 1e-10
    assert all(g.abs().max() < 1e30 for g in case.ref.base)


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == "dead_relu"], ids=ids)
def test_dead_relu_gradients_are_exactly_zero_behind_the_relu(c):
    case = bc.backward_case(*c)
    assert (case.hd[0] <= 0).all() and (case.vs >= 0).all()
    assert all((u <= 0).all() for u in case.ref.us) and case.ref.amb == []
    d_vol, d_ft, d_W1, d_W2, d_b2 = case.ref.base
    for g in (d_vol, d_W1, d_W2) + tuple(case.g32[i] for i in (0, 2, 3)):
        assert not g.any()                                # all-zero in both precisions
    assert d_ft.abs().max() > 0 and d_b2.abs().max() > 0 and case.e_ref[1] > 0 and case.e_ref[4] > 0
    # d feat_tgt[b] = sum_n g[b, n] / 64 * (b2 / |b2|) at every position
    q = bc.oc.dead_relu_column(case.hd)
    want = (case.gs.double().sum(dim=1) / 64)[:, None, None] * q[None, :, None].expand(case.B, 32, 64)
    assert (d_ft - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("kind,key", bc.ROTGRAD, ids=["%s-%s" % c for c in bc.ROTGRAD])
def test_rotation_gradient_cases_leave_few_hypotheses_out(kind, key):
    """The rotation-gradient cases under the rules of tests/test_gpu_rotation_grad.py, unchanged: at most 5 % of the hypotheses
    are ambiguous (none of a case of fewer than 20), and stock torch in fp32 on the CPU meets PARITY_BAR on the rest."""
    from .test_gpu_rotation_grad import PARITY_BAR, check_ambiguous, hyp_err, ref_rotation_grad
    case = bc.backward_case(kind, 3, S3[key], True)
    ref, amb = ref_rotation_grad(*case.args, scale=case.scale)
    f32, _ = ref_rotation_grad(*case.args, dtype=torch.float32, scale=case.scale)
    left = check_ambiguous(case.name, amb, None)
    err = hyp_err(f32, ref)
    print("%-46s %d hypotheses, %d ambiguous; torch fp32: median %.2g max %.2g" % (
        case.name, amb.numel(), left, err[~amb].median().item(), err[~amb].max().item()))
    assert torch.isfinite(ref).all() and err[~amb].max().item() <= PARITY_BAR
    if kind == "dead_relu":
        assert not ref.any() and not f32.any() and left == 0
    else:
        assert (ref.flatten(2).abs().max(dim=2).values > 0).all()


def test_a_flip_evaluated_on_its_hypothesis_is_the_flip_evaluated_on_the_batch():
    """bc.HypothesisKinkReference.delta against KinkReference.delta, on the near-kink pre-activations of two small cases."""
    seen = 0
    for c in (("plain", 3, 1, True), ("clamp", 3, S3["partial"], True), ("plain", 1, S1["partial"], False)):
        case = bc.backward_case(*c)
        for b, idx in case.ref.amb:
            # (the batch's delta is a difference of two whole gradients: good to fp64 rounding of THEIR size)
            for x, y, g in zip(case.ref.delta(b, idx), bc.KinkReference.delta(case.ref, b, idx), case.ref.base):
                assert x.shape == y.shape == g.shape and (x - y).abs().max() <= 1e-13 * g.abs().max()
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_d_b2_does_not_cancel(c):
    """Condition (e), bc.chain_sd: DB2_Z = 3 standard deviations of the difference of two float-atomic evaluations of d b2 fit
    inside SAVED_RTOL, which the GPU file holds the saved and the recomputing backward to, unchanged.  The diagnostic is zero
    for the three gradients that are no chains over hypotheses and enters no bar."""
    case = bc.backward_case(*c)
    sd = bc.chain_sd(case)
    print("%-46s chain sd / max: d feat_tgt %.2e (e_ref %.2e)  d b2 %.2e (e_ref %.2e)  seed steps %d" % (
        case.name, sd[1], case.e_ref[1], sd[4], case.e_ref[4], case.seed_steps))
    assert sd[0] == sd[2] == sd[3] == 0 and sd[1] > 0 and sd[4] > 0
    assert bc.DB2_Z * 2 ** 0.5 * sd[4] <= bc.SAVED_RTOL == 5e-6
    assert case.bars()[0] == [min(bc.GRAD_RTOL, bc.PARITY_FACTOR * e) for e in case.e_ref]


def test_the_xcd_remap_branches_the_cases_reach():
    """xcd_residue's remap of blockIdx.x by gx of (head, saved, w1, vol, du): B = 3 (gx = 85, 43, 22, three rows) takes the
    early return, B = 2 at vol_turn the even split with two rows, B = 1 the even split at gx = 256 -- and at du_turn, N = 257,
    the ragged one (gx = 65, 33, 65, 129: the first gx % 8 XCDs take one residue more), which needs one row and 16 <= gx, gx % 8 != 0."""
    remap = lambda B, N: [bc.xcd_remap(*bc.grid(CU, B, N, bc.PER_WG[p])) for p in KERNELS]
    assert [bc.grid(CU, 1, 257, bc.PER_WG[p])[0] for p in KERNELS] == [65, 33, 65, 129, 256]
    assert remap(1, S1["du_turn"]) == ["ragged", "ragged", "ragged", "ragged", "even"]
    assert remap(1, S1["head_turn"]) == ["even", "ragged", "even", "even", "even"] and remap(1, S1["all_ragged"]) == ["even"] * 5
    assert remap(1, S1["partial"]) == ["identity"] * 5
    assert all(remap(3, S3[k]) == ["identity"] * 5 for k in S3)
    assert remap(2, S2["vol_turn"]) == ["identity", "identity", "identity", "even", "even"]
    assert [bc.xcd_residue(x, 65, 1) for x in (0, 1, 2, 8, 9, 64)] == [0, 9, 17, 1, 10, 8]


def test_the_recorded_yardsticks_are_the_measured_range():
    """The docstring of tests/backward_cases.py records the range of e_ref over the well-posed cases."""
    lo, hi = bc.YARDSTICK_RANGE
    es = [e for c in CASES for e in bc.backward_case(*c).e_ref if e > 0]
    print("e_ref over %d gradients: %.2e .. %.2e" % (len(es), min(es), max(es)))
    assert lo <= min(es) and max(es) <= hi
