"""The backward of the fused scorer (csrc/ahv_backward.hip: score_backward_head_kernel, score_backward_head_saved_kernel, dW1 and
its reduce; csrc/ahv_bwd_volume.hip: the dV scatter; csrc/ahv_rotgrad.hip: the head-only pass and score_rotation_grad_kernel)
on random heads of every kind, un-normalised target features, the clamp branch of the head rule (csrc/ahv_bwd.h,
head_tile_backward) and every edge of the grid rule (backward_grid, csrc/ahv_launch.h), each gradient against the CPU fp64
autograd reference under the rule of tests/backward_cases.py: e_got <= min(GRAD_RTOL, 10 e_ref), e_ref being the CPU fp32
autograd gradients' own distance from fp64 on the same case.  Inputs, references, grid arithmetic and the clamp cases' gap
rule are tests/backward_cases.py's; the conditions the cases must meet are checked without a GPU in
tests/test_backward_cases_cpu.py.  The hypothesis counts follow from the device's CU count (256 on the MI355X: B = 3
1 / 7 / 86 / 171 / 341 / 680 / 681, B = 1 7 / 257 / 1025 / 2049, B = 2 257, B = 257 1 / 9).

Every case runs the recomputing backward, then the training forward (scores equal to the inference launch's bit for bit)
and the saved backward; both gradient sets are held to the case's bars, d vol_src per sample as well, and to each other
within SAVED_RTOL, unchanged, for all five gradients.

e_got / e_ref on the MI355X, both backwards (a run with -s prints every figure; e_ref is 2e-7 ... 4.3e-6, see
tests/backward_cases.py):

    d vol_src   0.84 - 1.71 over all 25 cases, per sample 0.59 - 1.71;  d W1  0.84 - 1.44;  d W2  0.93 - 2.83
    d feat_tgt  N <= 9 (B = 1, 3, 257)                 0.91 - 1.47
                N = 86, 171, 257 (B = 3, 2, 1)         1.11 - 2.17   (dead_relu N = 171: 2.72)
                N = 341, 680, 681 (B = 3)              1.96 - 3.85
                B = 1: N = 1025 / N = 2049             3.17 - 3.72 / 5.59 (recomputing), 8.15 (saved)
    d b2        0.07 - 1.94, but B = 257, N = 9: plain 1.65, 1.87, clamp 4.05, 3.77
    dead_relu   d vol_src, d W1, d W2: all-zero bits from both backwards, e_got = e_ref = 0
    saved against recomputing   d vol_src <= 6.8e-7, d W1 <= 2.7e-7, d W2 <= 1.4e-6, d feat_tgt <= 2.6e-6 (B = 1, N = 2049),
                                d b2 <= 2.6e-6 (clamp, B = 257, N = 9) of the largest entry
    rotation gradient           max err 1.4e-6 (plain, N = 86), 2.4e-6 (no_bias), 1.9e-6 (clamp), 1.6e-6 (plain, N = 341), 0 (dead_relu)
                                against PARITY_BAR = 2.5e-5; clamp: the same bits from one call and from two

Only d feat_tgt and d b2 leave the neighbourhood of 1, and they grow with N: both are sums over the hypotheses by float atomics
into single words, a chain of N (B N) adds where the CPU reference reduces blockwise (bc.chain_sd models it; the model enters no
bar).  The narrowest margin is d feat_tgt of the saved backward at B = 1, N = 2049, whose e_ref, 2.6 - 2.8e-7, is the smallest of
any non-trivial case: 5.5 - 8.2 of the 10 it is allowed over five runs, the order of the atomics moving it from run to run.  If a
run exceeds the bar there, the issue's remedy applies to that gradient of that case: establish that it is the chain, and state an
allowance derived in fp64 from the reference's terms beside its bar.  d b2 is held to SAVED_RTOL between the two backwards on cases
whose d b2 does not cancel (condition (e) of tests/backward_cases.py, on the reference alone).

Checked against two deliberately wrong builds (not kept; each only skips work or changes arithmetic), this file as it stands run
once on each:
 1. c3 of head_tile_backward computed without the `clamped` select.  The five tests on clamp cases fail (d vol_src 0.16 - 0.31 of
    its largest entry, the rotation gradient 0.62) and the other 23 pass.
 2. the hypothesis walk of kernel 1 (both instances) and of the dV kernel stopped after one turn.  The 13 tests with a hypothesis
    past a first turn fail -- d vol_src alone where only the dV kernel has a second turn (vol_turn, every kind but dead_relu;
    B = 2, N = 257), every gradient where kernel 1 has one too (head_turn, all_exact, all_ragged, B = 257 with N = 9), and the
    rotation gradient of plain-head_turn (hypothesis 340 of every sample, in the head-only pass' second turn, error 1.0) -- and
    the other 15 pass, with dead_relu at vol_turn, whose d vol_src is zero with or without a second turn.
"""
import pytest
import torch

from . import backward_cases as bc
from .backward_reference import relerr
from .test_gpu_backward import SAVED_RTOL, both_backwards
from .test_gpu_rotation_grad import PARITY_BAR, check_ambiguous, hyp_err, ref_rotation_grad

pytestmark = pytest.mark.gpu


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


def check_case(ops, dev, case):
    """Both backwards of one case: the bars, the two sets against each other, the exact zeros of dead_relu."""
    args = [t.to(dev) for t in case.args]
    want, saved = both_backwards(ops, *args)            # asserts: training scores == inference scores, bit for bit
    for tag, got in (("recomputing", want), ("saved", saved)):
        bc.accept_grads(got, case, "%s, %s" % (case.name, tag))
        if case.kind == "dead_relu":
            for i in (0, 2, 3):                         # nothing passes the ReLU: d vol_src, d W1 and d W2 are all-zero bits
                assert not got[i].view(torch.int32).any(), "%s, %s: d %s has a set bit" % (case.name, tag, bc.GRAD_NAMES[i])
    between = [relerr(a, b.double()) for a, b in zip(saved, want)]
    print("%-66s saved against recomputing: %s" % (case.name, " ".join("%.1e" % e for e in between)))
    assert max(between) < SAVED_RTOL, (case.name, dict(zip(bc.GRAD_NAMES, between)))


GRID = [(3, k) for k in bc.GRID_B3] + [(1, k) for k in bc.GRID_B1]


@pytest.mark.parametrize("B,key", GRID, ids=["B%d-%s" % c for c in GRID])
def test_gradients_at_every_grid_edge_against_fp64(ops, dev, cu, B, key):
    """plain head; B = 3 with R per sample at every name of bc.sizes, B = 1 with R shared (gx up to cu, r_batch_stride 0; at
    du_turn, N = cu + 1, the one row of workgroups has a gx that is no multiple of 8: xcd_residue's ragged remap)."""
    check_case(ops, dev, bc.backward_case("plain", B, bc.sizes(cu, B)[key], B > 1))


@pytest.mark.parametrize("k", range(2))
def test_gradients_of_many_samples_against_fp64(ops, dev, cu, k):
    """B = cu + 1 samples with a shared R: gx = 1 and workgroup row 0 walks samples 0 and cu, re-staging the volume, the
    target fragments and d feat_tgt between them.  The per-sample measure of d vol_src covers sample cu."""
    B, Ns = bc.many_samples(cu)
    case = bc.backward_case("plain", B, Ns[k], False)
    assert case.B - 1 == cu and case.ref.base[0][cu].abs().max() > 0
    check_case(ops, dev, case)


KINDS = [(kind, k) for kind in bc.OTHER_KINDS for k in bc.KIND_SIZES]


@pytest.mark.parametrize("kind,key", KINDS, ids=["%s-%s" % c for c in KINDS])
def test_gradients_of_every_head_kind_against_fp64(ops, dev, cu, kind, key):
    """B = 3, R per sample.  dead_relu: d vol_src, d W1 and d W2 are all-zero bits, d feat_tgt and d b2 meet their bars.
    clamp: about half of the columns of almost every hypothesis take the clamp branch of head_tile_backward."""
    check_case(ops, dev, bc.backward_case(kind, 3, bc.sizes(cu, 3)[key], True))


@pytest.mark.parametrize("which", ["shared", "many_samples"])
def test_clamp_gradients_with_a_shared_set_and_many_samples(ops, dev, cu, which):
    """clamp at B = 2 with one shared set (a second turn of the dV kernel), and at B = cu + 1, N = 9."""
    if which == "shared":
        case = bc.backward_case("clamp", 2, bc.sizes(cu, 2)["vol_turn"], False)
    else:
        case = bc.backward_case("clamp", bc.many_samples(cu)[0], 9, False)
    check_case(ops, dev, case)


# ---- the rotation gradient -------------------------------------------------------------------------------------------------
def rotation_grad(ops, dev, case, lo=None, hi=None):
    vs, ft, R, W1, W2, b2, gs = (t.to(dev) for t in case.args)
    if lo is not None:
        R, gs = R[..., lo:hi, :, :].contiguous(), gs[:, lo:hi].contiguous()
    return ops.score_rotation_grad(vs, ft, R, W1, W2, b2, gs)


@pytest.mark.parametrize("kind,key", bc.ROTGRAD, ids=["%s-%s" % c for c in bc.ROTGRAD])
def test_rotation_gradient_of_every_head_kind_against_fp64(ops, dev, cu, kind, key):
    """ops.score_rotation_grad, B = 3, R per sample; du_turn: one hypothesis into the second turn of the head-only pass.
    The reference, the error measure, the cap on what may be left out and PARITY_BAR are tests/test_gpu_rotation_grad.py's."""
    case = bc.backward_case(kind, 3, bc.sizes(cu, 3)[key], True)
    ref, amb = ref_rotation_grad(*case.args, scale=case.scale)
    left = check_ambiguous(case.name, amb, None)
    got = rotation_grad(ops, dev, case)
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all()
    err = hyp_err(got, ref)
    worst = err[~amb].max().item()
    print("%-66s rotation gradient: %d hypotheses, %d ambiguous, max err %.3g (median %.3g), bar %.3g" % (
        case.name, amb.numel(), left, worst, err[~amb].median().item(), PARITY_BAR))
    assert worst <= PARITY_BAR, (case.name, worst)
    if kind == "dead_relu":
        assert not ref.any() and not got.view(torch.int32).any()      # exact zeros
    if kind == "clamp":                                               # grad_R[b][n] does not depend on the cut into calls
        cut = case.N // 2
        parts = torch.cat([rotation_grad(ops, dev, case, 0, cut), rotation_grad(ops, dev, case, cut, case.N)], dim=1)
        assert torch.equal(got, parts)
