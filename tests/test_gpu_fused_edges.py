"""The fused scorer (csrc/ahv_score.hip: score_hypotheses_dual_kernel<SPLIT, TGT>, score_hypotheses_train_kernel,
coarse_to_fine_kernel) at every launch plan and head regime, every score against the CPU fp64 reference under the rule of
tests/oplevel_cases.py: e_got <= 4 e_ref, e_ref being the CPU fp32 reference's own distance from fp64 on the same case.
Inputs, references and the plan arithmetic are tests/fused_cases.py's; the hypothesis counts follow from the device's CU count
(256 on the MI355X: B = 1 512 / 513 / 2048 / 2049 / 2560 / 2561, B = 3 170 / 171 / 680 / 681 / 850 / 851), and every case
first asserts that the launch takes the plan it is meant to take.

e_got / e_ref on the MI355X (a run with -s prints them and a digest of every case's bytes; e_ref is 0.7 - 1.6e-7 for the
scores of the cases with hundreds of draws; two / one = forward_3d2d + score_hypotheses / verify_pair):

    plain, B = 1, shared R    N = 1  2  7 (few draws)           two 1.00 1.00 0.63   one 8.00 1.00 0.54   (of their bar: <= 0.40)
                              N = 512 513 2048 2049 2560 2561   two 0.64 0.70 0.65 0.66 0.60 0.59   one 0.71 0.73 0.77 0.62 0.59 0.75
    plain, B = 3, per sample  N = 7 | 170 171 681 851           two 0.62 | 0.70 0.72 0.64 0.70      one 0.62 | 0.76 0.72 0.71 0.68
    no_bias   N = 170 171 850                                   two 0.99 0.95 1.03   one 1.11 0.95 1.11
    clamp     N = 170 171 850                                   two 0.97 1.00 1.34   one 1.09 1.25 1.12
    golden    N = 170 171 850                                   two 0.98 1.05 0.86   one 1.19 1.20 0.86
    dead_relu N = 170 171 850 (few draws)                       two 0.50 0.00 1.00   one 0.00 0.50 1.00   (0 - 2 ulp(1-) from 1)
    B = 257, shared R         plain N = 2 5 9 | clamp N = 5     two 0.84 0.74 0.68 | 1.03   one 0.78 0.81 0.75 | 1.30
    target features           forward_3d2d 0.32 - 1.55, in-launch (verify_pair) 0.41 - 1.55, coarse_to_fine 1.21, 1.78
    training forward          N = 1 7 680 683                   plain 0.47 0.62 0.66 0.56   clamp 0.62 1.27 1.06 1.07
    no_teams (fp32)           N = 1 7 680 683                   plain 0.47 0.62 0.66 0.56   no_bias 1.90 1.85 1.11 1.09
                                                                clamp 0.62 1.27 1.06 1.07   golden 1.82 0.85 1.03 0.88   dead_relu 0 - 1.00
    split-f16, e_split/e_ref  N = 1 7 680 683                   plain 0.60 0.75 0.64 0.57   no_bias 1.00 1.81 1.10 1.21
                                                                clamp 0.62 1.08 1.39 1.28   golden 1.19 0.89 0.75 0.83   dead_relu 0 - 1.00
                              (e_split <= 1.31 e_fp32kernel throughout; the rule is 4 e_fp32kernel + 1e-7)
    coarse_to_fine, B = 2     N = 1025, N2 = 1027               plain coarse 0.63 fine 0.75   clamp coarse 1.12 fine 0.90
    finite part of the flagged target features                  1.00 (verify_pair), 1.00 (coarse_to_fine)

Every class with hundreds of draws meets 4 e_ref with a factor of three to spare.  The few-draw cases (fewer than 64 scores, or
dead_relu, whose scores are all one number) have no such yardstick: e_ref is there the largest of a handful of draws of the
reference's rounding error, and was 6.6e-9 for the single score of B = 1, N = 1 (verify_pair: 5.3e-8, under one ulp of the
score, ratio 8.00) and 0 or 2.2e-16 for the first dead_relu heads drawn.  For them the bar is 4 e_ref + fc.rsq_allowance: what the
1-ulp v_rsq_f32 of d * rsq(max(|v|^2, 1e-24)) can cost where the reference divides by a correctly rounded sqrt, 2^-23 mean_p |c_p|
from the fp64 reference's own per-position terms (3e-8 to 1.2e-7), derived in fused_cases.py and fitted to nothing; and a
dead_relu head is the first of its seeds whose fp32 reference is not the correctly rounded fp64 value (e_ref >= 2^-25).

Found by test_target_features_keep_a_nan_norm: team 1's target prologue clamped the norm with fmaxf, which drops a NaN norm, and
left +-inf in 18 of the 96 elements the reference makes NaN in the features verify_pair and coarse_to_fine return (fixed: the
select of clamped_norm, csrc/ahv_ops.hip, spelled in place).  The test fails on the parent commit; every finite case of this file
has the parent's bytes (90 digests of scores and features compared between the two builds).

Checked against three deliberately wrong builds (not kept; arithmetic changes only), this file and tests/test_gpu_parity.py +
tests/test_gpu_verify.py run once on each:
 1. 1e-24f -> 1.21e-24f in hyp_score_tail alone.  Here: every clamp case that has lone waves fails (e_got ~2e-2: lone_first,
    tail_team_last, B = 257 N = 5, the training forward, no_teams, split-f16 and coarse_to_fine; clamp-teams_last, all teams,
    passes).  The old files: 81 passed.
 2. one bias channel times (1 + 2^-14) in load_dual_frags.  Here: 31 of 61 fail -- every plain, golden and dead_relu case
    (scores at 4.4 - 51 e_ref, target features at 7.6 - 650), the NaN-norm test's finite elements; no_bias and clamp (b2 = 0)
    pass.  The old files: no comparison with a reference fails (SCORE_RTOL holds); 16 kernel-against-kernel tests do
    (verify_pair equals two launches, bit for bit; the forward_3d2d paths against each other), because the fragment is not
    loaded the same way by every kernel.
 3. inv of the in-launch target features times (1 + 2^-15).  Here: verify_pair and coarse_to_fine fail in every case (scores
    above 100 e_ref), forward_3d2d + score_hypotheses, the training forward and split-f16 pass.  The old files: 23
    kernel-against-kernel tests fail (verify_pair against two launches, team tails against single waves) and
    test_verify_pair_config1_golden_and_oracle; SCORE_RTOL holds.
"""
import hashlib

import pytest
import torch

from . import fused_cases as fc

pytestmark = pytest.mark.gpu
ENTRIES = ("forward_3d2d + score_hypotheses", "verify_pair")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()  # raises if libahv_hip.so is missing: no fallback
    return ahv.ops


@pytest.fixture(scope="module")
def cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def launch(ops, dev, case, entry, vol_tgt=None, **kw):
    """(scores, best, idx, feat_tgt) on the CPU through one of the two entry points."""
    vs, vt, R = (t.to(dev) for t in (case.vol_src, case.vol_tgt if vol_tgt is None else vol_tgt, case.R))
    hd = tuple(t.to(dev) for t in case.hd)
    if entry == ENTRIES[0]:
        ft = ops.forward_3d2d(vt, *hd)
        scores, key = ops.score_hypotheses(vs, ft, R, *hd, **kw)
    else:
        scores, key, ft = ops.verify_pair(vs, vt, R, *hd, want_feat_tgt=True, **kw)
    best, idx = ops.unpack_best(key)
    return scores.cpu(), best.cpu(), idx.cpu(), ft.cpu()


def check_case(ops, dev, cu, case, entries=ENTRIES):
    """The plan, then per entry point: scores and target features under oc.accept, the key rule, the bytes' digest."""
    B, N = case.B, case.N
    assert ops.score_plan(B, N) == fc.plan(B, N, cu, True), "%s takes another plan" % case.name
    for entry in entries:
        what = "%s, %s" % (case.name, entry)
        scores, best, idx, ft = launch(ops, dev, case, entry)
        assert scores.shape == (B, N) and ft.shape == (B, 32, 64)
        print("%-74s sha256 %s" % (what, digest(scores, ft)))
        fc.accept_scores(scores, case, what)
        fc.accept(ft, case.ft32, case.ft64, what + ": feat_tgt")
        clear = fc.check_key(scores, best, idx, case.r64, fc.bar(case)[0], what)
        if case.kind == "dead_relu":
            off = (scores.double() - 1.0).abs().max().item() / 2.0 ** -24
            print("%-74s worst score %.2f ulp(1-) from 1; arg-max clear in %d of %d samples" % (what, off, clear, B))


# ---- every launch plan -----------------------------------------------------------------------------------------------------
PLANS_B1 = ["one", "pair", "teams_odd", "teams_last", "lone_first", "round_exact", "tail_team_first", "tail_team_last",
            "tail_lone_first"]
PLANS_B3 = ["teams_odd", "teams_last", "lone_first", "tail_team_first", "tail_lone_first"]
EVERY_PLAN = [(1, k) for k in PLANS_B1] + [(3, k) for k in PLANS_B3]


@pytest.mark.parametrize("B,key", EVERY_PLAN, ids=["B%d-%s" % c for c in EVERY_PLAN])
def test_scores_every_plan_against_fp64(ops, dev, cu, B, key):
    """plain head; B = 1 with R shared, B = 3 with R per sample; both entry points, scores, target features and keys."""
    check_case(ops, dev, cu, fc.fused_case("plain", B, fc.sizes(cu, B)[key], B > 1))


EVERY_KIND = [(kind, k) for kind in ("no_bias", "dead_relu", "clamp", "golden") for k in ("teams_last", "lone_first", "tail_team_last")]


@pytest.mark.parametrize("kind,key", EVERY_KIND, ids=["%s-%s" % c for c in EVERY_KIND])
def test_scores_every_head_kind_against_fp64(ops, dev, cu, kind, key):
    """B = 3, R per sample; teams only, lone waves only, and both.  clamp: half of the hot loop's columns take the clamp of
    d * rsq(max(|v|^2, 1e-24)); dead_relu: every score is 1."""
    check_case(ops, dev, cu, fc.fused_case(kind, 3, fc.sizes(cu, 3)[key], True))


@pytest.mark.parametrize("kind,k", [("plain", 0), ("plain", 1), ("plain", 2), ("clamp", 1)])
def test_scores_many_samples_against_fp64(ops, dev, cu, kind, k):
    """B = cu + 1 samples with a shared R: gx = 1 everywhere and one workgroup loops over two samples."""
    B, Ns = fc.many_samples(cu)
    check_case(ops, dev, cu, fc.fused_case(kind, B, Ns[k], False))


# ---- launches without teams ------------------------------------------------------------------------------------------------
def no_team_case(ops, cu, kind, k, **flags):
    N = fc.no_team_sizes(cu, 3)[k]
    case = fc.fused_case(kind, 3, N, True)
    assert ops.score_plan(3, N, **flags) == fc.plan(3, N, cu, False), "%s takes another plan" % case.name
    return case


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("kind", ["plain", "clamp"])
def test_training_forward_against_fp64(ops, dev, cu, kind, k):
    """score_hypotheses_train_kernel (plan_score_launch without teams), B = 3, R per sample."""
    case = no_team_case(ops, cu, kind, k, no_teams=True)
    hd = tuple(t.to(dev) for t in case.hd)
    ft = ops.forward_3d2d(case.vol_tgt.to(dev), *hd)
    scores, ws = ops.score_hypotheses_train(case.vol_src.to(dev), ft, case.R.to(dev), *hd)
    print("%-74s sha256 %s" % (case.name + ", training forward", digest(scores)))
    fc.accept_scores(scores, case, case.name + ", training forward")


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("kind", fc.KINDS)
def test_split_f16_on_random_heads(ops, dev, cu, kind, k):
    """The split-f16 kernel is not IEEE fp32 by design and keeps the rule of tests/test_gpu_split.py against the same fp64
    truth: e_split < 4 e_fp32kernel + 1e-7; its e_split / e_ref is printed beside it.  clamp is the case that matters: the
    clamp applies after the three power-of-two prescales are undone (ahv_split.h, exp_sum).  The fp32 kernel runs with
    no_teams here, under oc.accept: the same plan for both."""
    case = no_team_case(ops, cu, kind, k, split_f16=True)
    what = case.name + ", split-f16"
    s16, best, idx, _ = launch(ops, dev, case, ENTRIES[0], split_f16=True)
    s32, _, _, _ = launch(ops, dev, case, ENTRIES[0], no_teams=True)
    print("%-74s sha256 %s (no_teams fp32 %s)" % (what, digest(s16), digest(s32)))
    fc.accept_scores(s32, case, case.name + ", no_teams")
    e16, e_ref = fc.errors(s16, case.r32, case.r64)
    e32, _ = fc.errors(s32, case.r32, case.r64)
    print("%-74s e_split %.3e  e_fp32kernel %.3e  e_ref %.3e  e_split/e_ref %.2f" % (what, e16, e32, e_ref, e16 / e_ref))
    assert e16 < 4 * e32 + 1e-7
    want, want_idx = torch.max(s16, dim=1)
    assert torch.equal(best, want) and torch.equal(idx, want_idx)


# ---- coarse to fine --------------------------------------------------------------------------------------------------------
def c2f(ops, dev, case, D, vol_tgt=None):
    hd = tuple(t.to(dev) for t in case.hd)
    out = ops.coarse_to_fine(case.vol_src.to(dev), (case.vol_tgt if vol_tgt is None else vol_tgt).to(dev), case.R.to(dev),
                             D.to(dev), *hd, want_scores=True, want_feat_tgt=True)
    assert not out["state"].gave_up()
    return {k: v.cpu() for k, v in out.items() if k != "state"}


@pytest.mark.parametrize("kind", ["plain", "clamp"])
def test_coarse_to_fine_stages_against_fp64(ops, dev, cu, kind):
    """coarse_to_fine_kernel, B = 2, R per sample: stage 0 is a round + one hypothesis by a team, stage 1 a round + a team
    tail of three on stage 0's grid.  The fine reference is evaluated at R[coarse_idx] @ D with coarse_idx taken from the
    launch (checked by the key rule), the product in fp32 for ref32 and in fp64 for ref64."""
    B = 2
    N, N2 = fc.c2f_sizes(cu, B)
    case, D = fc.c2f_case(kind, B, N, N2)
    gx, gy, n_main, n_main2 = fc.c2f_plan(B, N, N2, cu)
    assert ops.score_plan(B, N) == (gx, gy, n_main) and 0 < N - n_main <= 2 * gx and 0 < N2 - n_main2 <= 2 * gx
    out = c2f(ops, dev, case, D)
    what = case.name + ", coarse_to_fine"
    print("%-74s sha256 %s" % (what, digest(out["coarse_scores"], out["fine_scores"], out["feat_tgt"])))
    fc.accept_scores(out["coarse_scores"], case, what + ": coarse")
    fc.accept(out["feat_tgt"], case.ft32, case.ft64, what + ": feat_tgt")
    fc.check_key(out["coarse_scores"], out["coarse_score"], out["coarse_idx"], case.r64, fc.bar(case)[0], what + ": coarse")
    f32, f64 = fc.fine_refs(case, D, out["coarse_idx"])
    e_fine = fc.errors(f32, f32, f64)[1]
    fc.accept(out["fine_scores"], f32, f64, what + ": fine")
    fc.check_key(out["fine_scores"], out["fine_score"], out["fine_idx"], f64, fc.MARGIN * e_fine, what + ": fine")
    want = torch.stack([case.R[b, int(out["coarse_idx"][b])].double() @ D[int(out["fine_idx"][b])].double() for b in range(B)])
    assert (out["R_pred"].double() - want).abs().max() <= 8 * 2.0 ** -24     # a 3-term fp32 product of entries <= 1


# ---- a NaN norm on the target side -----------------------------------------------------------------------------------------
def test_target_features_keep_a_nan_norm(ops, dev, cu):
    """oc.inf_column_case in the middle target of B = 3: one column holds +-inf beside NaN before it is normalised, so its
    norm is NaN; F.normalize's clamp_min keeps the NaN and the reference's column is NaN throughout.  The in-launch target
    features of verify_pair and coarse_to_fine clamped with fmaxf, which drops the NaN and left +-inf in the column."""
    N, N2 = fc.c2f_sizes(cu, 3)
    case = fc.nan_norm_case(N)
    D = fc.haar(N2, 77)
    m, rest = case.flagged, [0, 2]
    nan32 = torch.isnan(case.ft32)
    assert torch.equal(nan32, torch.isnan(case.ft64)) and nan32[m].any() and not nan32[rest].any()
    assert ops.score_plan(3, N) == fc.plan(3, N, cu, True)

    def check(what, feat, feat_clean, scores, scores_clean):
        print("%-74s %d inf and %d NaN where the reference has %d NaN" % (
            what, torch.isinf(feat[m]).sum().item(), torch.isnan(feat[m]).sum().item(), nan32[m].sum().item()))
        for s, c in zip(scores, scores_clean):
            assert torch.isnan(s[m]).all(), what + ": finite score of the flagged sample"
            assert torch.isfinite(c).all() and torch.equal(s[rest], c[rest]), what + ": another sample's scores changed"
        assert torch.isfinite(feat_clean).all() and torch.equal(feat[rest], feat_clean[rest]), what + ": another sample's features changed"
        fc.accept(feat[m:m + 1], case.ft32[m:m + 1], case.ft64[m:m + 1], what + ": finite elements of the flagged features")
        assert torch.equal(torch.isnan(feat), nan32), what + ": NaN mask differs from the reference's"

    s, _, _, ft = launch(ops, dev, case, ENTRIES[1])
    sc, _, _, ftc = launch(ops, dev, case, ENTRIES[1], vol_tgt=case.vol_tgt_clean)
    fc.accept(s[rest], case.r32[rest], case.r64[rest], case.name + ", verify_pair: scores of the clean samples")
    check(case.name + ", verify_pair", ft, ftc, [s], [sc])
    o, oc_ = c2f(ops, dev, case, D), c2f(ops, dev, case, D, vol_tgt=case.vol_tgt_clean)
    check(case.name + ", coarse_to_fine", o["feat_tgt"], oc_["feat_tgt"], [o["coarse_scores"], o["fine_scores"]],
          [oc_["coarse_scores"], oc_["fine_scores"]])
