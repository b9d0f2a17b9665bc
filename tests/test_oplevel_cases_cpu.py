"""The conditions the cases of tests/oplevel_cases.py must meet for tests/test_gpu_oplevel_edges.py to mean what it says,
checked on the CPU references alone (sized for the MI355X's 256 CUs)."""
import time

import pytest
import torch

from . import oplevel_cases as oc

CU = oc.CU_MI355X
PER_PATH = [64, oc.sizes(CU)["mid_second_pass"], oc.sizes(CU)["dual_first"]]   # one M per forward_3d2d kernel


def test_sizes_land_on_their_paths():
    s = oc.sizes(CU)
    assert (s["mid_first"], s["mid_second_pass"], s["mid_last"]) == (65, 1027, 4095)
    assert (s["dual_first"], s["dual_lone_third_pass"], s["dual_ragged_third_pass"]) == (4096, 4097, 4397)
    assert oc.rotate_sizes(CU) == {"fast": 3077, "generic": 8746}
    assert oc.score_sizes(CU)[-1] == (2, 4099)
    for cu in (64, 255, 257, 304):   # other devices: the checks inside sizes() say so instead of testing another path
        try:
            oc.sizes(cu)
        except AssertionError:
            assert cu < 256
        else:
            assert cu >= 256


@pytest.mark.parametrize("M", PER_PATH)
def test_clamp_case_has_both_populations(M):
    case = oc.forward_case(M, "clamp")
    assert not case.args[3].any()
    clamped, free = oc.clamp_masks(case)
    share = clamped.float().mean().item()
    assert 0.1 <= share <= 0.9, share
    norms = case.r64.norm(dim=1)
    assert (norms[clamped[:, 0]] < 1).all() and (norms[free[:, 0]] - 1).abs().max() < 1e-9
    for where in (clamped, free, None):
        assert oc.errors(case.r32, case.r32, case.r64, where)[1] > 0


@pytest.mark.parametrize("M", PER_PATH)
def test_dead_relu_columns_are_the_normalised_bias(M):
    case = oc.forward_case(M, "dead_relu")
    x, W1, W2, b2 = case.args
    assert (W1 <= 0).all() and (x >= 0).all()
    column = torch.nn.functional.normalize(b2, dim=0)
    assert torch.equal(case.r32, column[None, :, None].expand(M, 32, 64))      # bit for bit
    assert (case.r64 - oc.dead_relu_column((W1, W2, b2))[None, :, None]).abs().max() < 1e-15
    assert oc.errors(case.r32, case.r32, case.r64)[1] > 0


FORWARD = [(m, "plain") for m in oc.sizes(CU)["small"] + tuple(v for k, v in oc.sizes(CU).items() if k != "small")]
FORWARD += [(m, kind) for m in PER_PATH for kind in ("no_bias", "golden")]       # clamp and dead_relu: the tests above
OTHERS = [("score_case",) + bn for bn in oc.score_sizes(CU)]
OTHERS += [("rotate_case", w, CU) for w in ("fast", "generic", "adjoint_per", "adjoint_shared")]


@pytest.mark.parametrize("make", [("forward_case",) + c for c in FORWARD] + OTHERS, ids=lambda c: "-".join(map(str, c)))
def test_every_case_has_a_yardstick_no_weaker_than_the_old_bar(make):
    """e_ref > 0; 4 e_ref is no looser than 1e-5 max|ref| (forward_3d2d: the plain and golden heads); inputs and both
    references of a case take under 5 s."""
    t0 = time.perf_counter()
    case = getattr(oc, make[0])(*make[1:])
    took = time.perf_counter() - t0
    assert oc.errors(case.r32, case.r32, case.r64)[1] > 0, case.name
    if case.kind in (None, "plain", "golden"):
        oc.assert_not_weaker(case.r32, case.r64, case.name)
    assert took < 5.0, "%s took %.1f s" % (case.name, took)


@pytest.mark.parametrize("M", PER_PATH)
def test_non_finite_cases_flag_part_of_an_item(M):
    x, bad, plan, hd, r32, r64 = oc.nonfinite_case(M)
    flagged = [m for m, _, _ in plan]
    assert M - 1 in flagged and len(set(flagged)) == 3
    assert sorted(int(b) & 0xFFFFFFFF for b in bad.view(torch.int32)[~torch.isfinite(bad)].tolist()) == sorted(
        (oc.QNAN, oc.PINF, oc.NINF))
    changed = (bad.view(torch.int32) != x.view(torch.int32)).flatten(1).sum(1)
    assert changed.sum() == 3 and (changed[flagged] == 1).all()
    nan32 = torch.isnan(r32)
    assert torch.equal(nan32, torch.isnan(r64))
    per_item = nan32.flatten(1).sum(1)
    assert (per_item > 0).all() and (per_item < 32 * 64).all()       # partial: some but not all positions
    assert torch.equal(nan32.any(1), nan32.all(1))                    # whole columns (all 32 channels of a position)
    assert oc.errors(r32, r32, r64)[1] > 0


@pytest.mark.parametrize("M", PER_PATH)
def test_inf_column_case_is_nan_throughout_its_columns(M):
    x, bad, m, hd, r32, r64 = oc.inf_column_case(M)
    assert (~torch.isfinite(bad)).sum() == 1 and torch.isinf(bad[m]).sum() == 1
    nan32 = torch.isnan(r32)
    assert torch.equal(nan32, torch.isnan(r64)) and not torch.isinf(r32).any() and not torch.isinf(r64).any()
    assert torch.equal(nan32.any(1), nan32.all(1)) and nan32.any(1).sum() == 3      # three whole columns
    # the column at (h, w) = (3, 5) is the one with two +inf hidden units: +-inf where W2's two weights agree in sign
    assert nan32[0, :, 3 * 8 + 5].all()


def test_adjoint_chain_allowance_restates_the_reference():
    case = oc.rotate_case("adjoint_shared", CU)
    sd, adds = oc.adjoint_chain_allowance(*case.args)        # checks its own sum against the fp64 autograd
    assert sd.shape == case.r64.shape and (sd > 0).all() and adds > 10000
    e_ref = oc.errors(case.r32, case.r32, case.r64)[1]
    # the chain dominates the allowance, and the allowance is small beside one hypothesis' contribution (~0.3)
    assert sd.max() > e_ref and oc.CHAIN_Z * sd.max() + oc.MARGIN * e_ref < 0.01


def test_score_nan_cases_are_clean_to_begin_with():
    case = oc.score_case(3, 5)
    assert torch.isfinite(case.r32).all() and (case.args[0].norm(dim=2) - 1).abs().max() < 1e-6
