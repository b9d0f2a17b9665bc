"""The conditions the cases of tests/fused_cases.py must meet for tests/test_gpu_fused_edges.py to mean what it says,
checked on the CPU references alone (sized for the MI355X's 256 CUs).  Nothing here measures a kernel."""
import pytest
import torch

from . import fused_cases as fc

CU = fc.CU_MI355X
S1, S3 = fc.sizes(CU, 1), fc.sizes(CU, 3)
NT3 = fc.no_team_sizes(CU, 3)
B_MANY, N_MANY = fc.many_samples(CU)
C2F = fc.c2f_sizes(CU, 2)

EVERY_PLAN = [("plain", 1, S1[k], False) for k in S1]
EVERY_PLAN += [("plain", 3, S3[k], True) for k in ("teams_odd", "teams_last", "lone_first", "tail_team_first", "tail_lone_first")]
EVERY_KIND = [(kind, 3, S3[k], True) for kind in ("no_bias", "dead_relu", "clamp", "golden")
              for k in ("teams_last", "lone_first", "tail_team_last")]
MANY = [("plain", B_MANY, n, False) for n in N_MANY] + [("clamp", B_MANY, 5, False)]
NO_TEAMS = [(kind, 3, n, True) for kind in fc.KINDS for n in NT3]
COARSE = [(kind, 2, C2F[0], True) for kind in ("plain", "clamp")]
CASES = EVERY_PLAN + EVERY_KIND + MANY + NO_TEAMS + COARSE
ids = lambda c: "-".join(map(str, c))


def test_plan_reproduces_the_table():
    assert [S1[k] for k in ("teams_last", "lone_first", "round_exact", "tail_team_first", "tail_team_last", "tail_lone_first")] == [
        512, 513, 2048, 2049, 2560, 2561]
    assert [S3[k] for k in ("teams_last", "lone_first", "round_exact", "tail_team_first", "tail_team_last", "tail_lone_first")] == [
        170, 171, 680, 681, 850, 851]
    assert (S1["one"], S1["pair"], S1["teams_odd"]) == (1, 2, 7)
    assert fc.plan(1, 7, CU, True) == (4, 1, 0) and fc.plan(1, 2049, CU, True) == (256, 1, 2048)
    assert fc.plan(3, 850, CU, True) == (85, 3, 680) and fc.plan(3, 851, CU, True) == (85, 3, 851)
    assert fc.plan(3, 681, CU, False) == (85, 3, 681) and fc.plan(1, 7, CU, False) == (2, 1, 7)
    assert NT3 == (1, 7, 680, 683) and (B_MANY, N_MANY) == (257, (2, 5, 9)) and C2F == (1025, 1027)
    assert fc.c2f_plan(2, 1025, 1027, CU) == (128, 2, 1024, 1024)
    for B in (1, 3):              # an odd CU count: G is no power of two for B = 1 either; sizes() checks every key with plan
        s = fc.sizes(250, B)
        G = 250 // B
        assert s["teams_last"] == 2 * G and s["tail_lone_first"] == 10 * G + 1
        assert fc.plan(B, s["tail_team_last"], 250, True) == (G, B, 8 * G)
        assert fc.plan(B, s["tail_team_last"], 250, False) == (G, B, 10 * G)
    fc.no_team_sizes(250, 3), fc.many_samples(250), fc.c2f_sizes(250)


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_every_case_has_a_finite_reference_and_a_yardstick_no_weaker_than_the_old_bar(c):
    case = fc.fused_case(*c)
    assert case.r32.shape == case.r64.shape == (case.B, case.N)
    assert torch.isfinite(case.r64).all() and torch.isfinite(case.r32).all()
    assert torch.isfinite(case.ft64).all() and fc.errors(case.ft32, case.ft32, case.ft64)[1] > 0
    assert case.e_ref() > 0, case.name
    fc.assert_not_weaker(case)          # MARGIN * e_ref (+ allowance) <= 1e-4 max(|ref64|, 1e-2) at the tightest element
    limit, A = fc.bar(case)
    if fc.few_draws(case):              # fewer than 64 scores, or dead_relu: one 1-ulp rsq per position, all one way
        assert case.B * case.N < 64 or case.kind == "dead_relu"
        assert 0 < A <= fc.RSQ_ULP * (1 + 1e-12) and limit == fc.MARGIN * case.e_ref() + A      # |c_p| <= 1: at most one ulp of 1
    else:
        assert A == 0 and limit == fc.MARGIN * case.e_ref()


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == "clamp"], ids=ids)
def test_clamp_cases_have_both_populations_in_every_hypothesis(c):
    case = fc.fused_case(*c)
    assert not case.hd[2].any()
    per_sample, per_hyp = fc.clamp_shares(case)
    assert (per_sample >= 0.25).all() and (per_sample <= 0.75).all(), per_sample
    assert (per_hyp > 0).all() and (per_hyp < 1).all(), (per_hyp.min().item(), per_hyp.max().item())
    # squares stay clear of the fp32 denormal range (1.2e-38): the smallest column norm is well above 1e-15
    assert case.src_norm.min() > 1e-14
    # no target column is clamped: unit norm, at scale 1
    assert (case.ft64.norm(dim=1) - 1).abs().max() < 1e-9
    assert case.vol_tgt.abs().max() > 1 and case.vol_src.abs().max() < 1e-10


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == "dead_relu"], ids=ids)
def test_dead_relu_scores_are_the_normalised_bias_against_the_target(c):
    case = fc.fused_case(*c)
    W1, W2, b2 = case.hd
    assert (W1 <= 0).all() and (case.vol_src >= 0).all() and (case.vol_tgt >= 0).all()
    q = fc.oc.dead_relu_column(case.hd)
    want = torch.einsum("c,bcp->bp", q, case.ft64).mean(-1)          # <b2/|b2|, f_tgt> averaged over positions
    assert (case.r64 - want[:, None]).abs().max() <= 1e-12
    assert (want - 1).abs().max() <= 1e-12                              # the target side is dead too
    assert case.e_ref() >= 2.0 ** -25                                   # the fp32 reference is not the nearest fp32 number


def test_inf_column_target_is_nan_in_whole_columns_and_in_every_score():
    assert fc.c2f_sizes(CU, 3) == (681, 683)
    case = fc.nan_norm_case(fc.c2f_sizes(CU, 3)[0])
    m = case.flagged
    assert m == 1 and case.B == 3
    assert (~torch.isfinite(case.vol_tgt)).sum() == 1 and torch.isinf(case.vol_tgt[m]).sum() == 1
    assert torch.isfinite(case.vol_tgt_clean).all() and torch.isfinite(case.vol_src).all()
    nan32, nan64 = torch.isnan(case.ft32), torch.isnan(case.ft64)
    assert torch.equal(nan32, nan64) and not torch.isinf(case.ft32).any() and not torch.isinf(case.ft64).any()
    assert not nan32[[0, 2]].any()
    assert nan32[m].all(0).sum() == 3 and torch.equal(nan32[m].any(0), nan32[m].all(0))   # 3 whole columns of 64, none partial
    for r in (case.r32, case.r64):
        assert torch.isnan(r[m]).all() and torch.isfinite(r[[0, 2]]).all()
    assert fc.errors(case.r32, case.r32, case.r64)[1] > 0 and fc.errors(case.ft32, case.ft32, case.ft64)[1] > 0
