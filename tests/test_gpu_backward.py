"""Backward of the fused scorer (ahv_score_hypotheses_backward_f32) against torch
autograd through the reference's op sequence (oracle/torch_ref.py, stock torch operators) evaluated in fp64.
Tolerance: gradients are sums over up to B*N hypotheses of fp32 terms -> 2e-4 of the largest entry.

ReLU has a kink: a pre-activation within fp32 rounding of zero (about one element in 5e6; a B = 2 x N = 1100 case
has 4.5e6 of them) makes an fp32 and an fp64 evaluation take different sub-gradients, which moves d vol / d W1 by
1e-3..1e-2 -- arithmetic, not implementation.  The comparison is therefore made against
the fp64 gradient for EVERY assignment of the ambiguous sub-gradients: the pre-activations the fp64 reference finds
within KINK_TAU of zero are listed, the reference gradient is evaluated with each of them flipped (the gradient
is affine in those indicator bits), the bits are fitted to the kernel's gradients by least squares and rounded, and
the kernel must match that one reference within the unchanged tolerance.  Cases with no ambiguous element (or that
already agree) reduce to the plain comparison."""
import numpy as np
import pytest
import torch

from . import rotation_families as fam
from .backward_reference import (GRAD_RTOL, KINK_MAX, KINK_TAU, KinkReference, kink_aware_errors, ref_scores,  # noqa: F401
                                 ref_scores_masked, relerr)
from .conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def make_case(ahv, dev, B, N, per_sample, seed):
    g = load_golden("score_n128")
    rng = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vs = t((rng.standard_normal((B, 16, 8, 8, 8)) * 1.1).astype(np.float32))
    ft = torch.nn.functional.normalize(t(rng.standard_normal((B, 32, 64)).astype(np.float32)), dim=1)
    R = ahv.rotations.haar_rotations_np(N * (B if per_sample else 1), seed + 1)
    R = t(R.reshape(B, N, 3, 3) if per_sample else R)
    gs = t(rng.standard_normal((B, N)).astype(np.float32))
    return vs, ft, R, t(g["W1"]), t(g["W2"]), t(g["b2"]), gs


@pytest.mark.parametrize("B,N,per_sample", [(1, 1, False), (1, 37, False), (2, 9, True), (3, 130, True), (2, 1100, False),
                                            (300, 2, True)])   # more samples than CUs: a workgroup walks several
def test_backward_matches_fp64_autograd(ops, ahv, dev, B, N, per_sample):
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, B, N, per_sample, 5 + B + N)
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    errs, n_amb, combo = kink_aware_errors(got, vs, ft, R, W1, W2, b2, gs)
    names = ["vol_src", "feat_tgt", "W1", "W2", "b2"]
    errs = dict(zip(names, errs))
    print(B, N, per_sample, {k: "%.1e" % v for k, v in errs.items()}, "near-kink pre-activations:", n_amb, "flipped:", combo)
    assert all(v < GRAD_RTOL for v in errs.values()), (errs, n_amb)


@pytest.mark.parametrize("B,N,per_sample", [(1, 1, False), (2, 9, True), (3, 130, True), (2, 1100, False), (5, 2048, True),
                                            (300, 3, True), (260, 17, False)])   # more samples than CUs
def test_saved_preactivations_backward_equals_the_recomputing_one(ops, ahv, dev, B, N, per_sample):
    """The training pair (ABI 2.3): ahv_score_hypotheses_train_f32 leaves every hypothesis' pre-activations in the workspace,
    ahv_score_hypotheses_backward_saved_f32 reads them instead of recomputing rotate_volume + the first projection.  Same
    scores as the inference launch bit for bit (the same accumulation chain), and the five gradients of the recomputing
    backward -- which the other tests hold to the fp64 reference -- to rounding (the head's arithmetic is the same code on
    the same values; the sums across hypotheses use float atomics in both)."""
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, B, N, per_sample, 31 + B + N)
    scores, ws = ops.score_hypotheses_train(vs, ft, R, W1, W2, b2)
    ref_scores, _ = ops.score_hypotheses(vs, ft, R, W1, W2, b2)
    assert torch.equal(scores, ref_scores)
    want = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs, workspace=ws)
    for a, b, name in zip(got, want, ("vol_src", "feat_tgt", "W1", "W2", "b2")):
        assert relerr(a, b.double()) < 5e-6, (name, relerr(a, b.double()))   # (measured <= 2.2e-6: the order of the float-atomic sums)


def test_autograd_function_uses_the_saved_forward_and_survives_a_second_backward(ops, ahv, dev):
    """ops.score_hypotheses_autograd / ops.score_hypotheses under autograd run the training forward; the workspace serves ONE
    backward, a second one (retain_graph) falls back on the recomputing kernels -- same gradients either way; the key that
    score_hypotheses returns beside differentiable scores is still torch.max's."""
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 2, 300, True, 91)
    leaves = [t.clone().requires_grad_(True) for t in (vs, ft, W1, W2, b2)]
    s = ops.score_hypotheses_autograd(leaves[0], leaves[1], R, leaves[2], leaves[3], leaves[4])
    g1 = torch.autograd.grad(s, leaves, grad_outputs=gs, retain_graph=True)
    g2 = torch.autograd.grad(s, leaves, grad_outputs=gs)
    want = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    for a, b, c in zip(g1, g2, want):
        assert relerr(a, c.reshape(a.shape).double()) < 2e-6 and relerr(b, c.reshape(b.shape).double()) < 2e-6
    s2, key = ops.score_hypotheses(leaves[0], leaves[1], R, leaves[2], leaves[3], leaves[4])
    assert s2.requires_grad and torch.equal(s2.detach(), s.detach())
    val, idx = ops.unpack_best(key)
    tv, ti = torch.max(s2.detach(), dim=1)
    assert torch.equal(idx, ti) and torch.equal(val, tv)


def test_saved_backward_poisons_a_non_finite_sample_only(ops, ahv, dev):
    """A sample with a NaN voxel goes through the forward's exact path, which keeps no accumulators: its saved pre-activations
    are NaN and so are its gradients; the finite sample beside it is untouched."""
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 2, 200, True, 92)
    clean = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    bad = vs.clone()
    bad[0, 3, 2, 5, 1] = float("nan")
    scores, ws = ops.score_hypotheses_train(bad, ft, R, W1, W2, b2)
    ref_scores, _ = ops.score_hypotheses(bad, ft, R, W1, W2, b2)
    assert torch.equal(torch.isnan(scores), torch.isnan(ref_scores)) and torch.equal(scores[1], ref_scores[1])
    got = ops.score_hypotheses_backward(bad, ft, R, W1, W2, b2, gs, workspace=ws)
    assert torch.isnan(got[0][0]).float().mean().item() > 0.9 and torch.isfinite(got[0][1]).all()
    assert relerr(got[0][1], clean[0][1].double()) < 2e-6


def test_backward_at_integer_sample_coordinates(ops, ahv, dev):
    """identity and the 24 cube rotations put EVERY sample coordinate exactly on an integer -- where the forward's
    point-mirror gather (quarters 3 and 2 reuse the set-up of 0 and 1, csrc/ahv_dual.h hat_mirror) picks the neighbouring
    base row with weights (0, 1) instead of (1, 0), while the dW1 / dV kernels evaluate all four quarters directly.  Same
    samples, so the five gradients must still be those of the fp64 reference; the 45-degree, scaled, non-orthonormal and
    zero matrices of the G3 fixture ride along (R is never assumed to be a rotation)."""
    g3 = load_golden("edge_rotations")
    vs, ft, _, W1, W2, b2, _ = make_case(ahv, dev, 2, 1, False, 77)
    R = torch.from_numpy(np.ascontiguousarray(g3["R"])).to(dev)
    gs = torch.from_numpy(np.random.RandomState(78).standard_normal((2, R.shape[0])).astype(np.float32)).to(dev)
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    errs, n_amb, combo = kink_aware_errors(got, vs, ft, R, W1, W2, b2, gs)
    assert all(v < GRAD_RTOL for v in errs), (errs, n_amb, combo)
    # and the forward at the same rotations, fused against the reference-generated scores of the fixture's own volume
    g1 = load_golden("score_n128")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s, _ = ops.verify_pair(t(g1["vol_src"]), t(g1["vol_tgt"]), R, W1, W2, b2, no_teams=True)
    ref = g3["scores"]
    assert float(np.max(np.abs(s.cpu().numpy() - ref) / np.maximum(np.abs(ref), 1e-2))) < 1e-4


@pytest.mark.parametrize("seed", [1101, 1102, 1103, 1106])
def test_backward_large_case_any_seed(ops, ahv, dev, seed):
    """B = 2 x N = 1100 on seeds whose plain fp64 comparison trips over a ReLU kink: the kink-aware reference must
    explain the kernel's gradients to the same tolerance (no seed picking)."""
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 2, 1100, False, seed)
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    errs, n_amb, combo = kink_aware_errors(got, vs, ft, R, W1, W2, b2, gs)
    print(seed, ["%.1e" % e for e in errs], "near-kink:", n_amb, "flipped:", combo)
    assert max(errs) < GRAD_RTOL, (errs, n_amb)


def test_autograd_function_trains_like_torch(ops, ahv, dev):
    """ops.score_hypotheses_autograd inside an infoNCE-style loss: same loss and gradients as the all-torch graph."""
    vs, ft, R, W1, W2, b2, _ = make_case(ahv, dev, 2, 64, True, 3)
    def loss_of(score_fn, leaves):
        s = score_fn(*leaves)
        logits = s / 0.1
        return -(torch.log_softmax(logits, dim=1)[:, :4].logsumexp(dim=1)).mean()
    a = [x.clone().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
    la = loss_of(lambda v, f, w1, w2, b: ops.score_hypotheses_autograd(v, f, R, w1, w2, b), a)
    la.backward()
    b_ = [x.double().clone().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
    lb = loss_of(lambda v, f, w1, w2, b: ref_scores(v, f, R.double(), w1, w2, b), b_)
    lb.backward()
    assert abs(la.item() - lb.item()) < 1e-5
    for x, y in zip(a, b_):
        assert relerr(x.grad, y.grad) < GRAD_RTOL


def test_backward_edge_cases(ops, ahv, dev):
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 2, 16, False, 9)
    # zero upstream gradient -> exact zeros; empty hypothesis set -> zeros of the right shapes
    z = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, torch.zeros_like(gs))
    assert all(float(t.abs().max()) == 0.0 for t in z)
    e = ops.score_hypotheses_backward(vs, ft, R[:0], W1, W2, b2, gs[:, :0])
    assert [tuple(t.shape) for t in e] == [(2, 16, 8, 8, 8), (2, 32, 64), (32, 384), (32, 32), (32,)]
    assert all(float(t.abs().max()) == 0.0 for t in e)
    with pytest.raises(RuntimeError):
        ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs[:, :3])
    # two calls agree to rounding (float atomics: not bitwise)
    a = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    b = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    assert all(relerr(x, y.double()) < 1e-5 for x, y in zip(a, b))


# ---- the dV scatter's two paths (tests/rotation_families.py; the lane-map model is tests/test_rmw_footprints_cpu.py) ----------
GRAD_NAMES = ("vol_src", "feat_tgt", "W1", "W2", "b2")
SAVED_RTOL = 5e-6       # saved against recomputing backward: the bar of test_saved_preactivations_backward_equals_the_recomputing_one
TWO_CALLS_RTOL = 1e-5   # "two calls agree to rounding": the bar of test_backward_edge_cases


def family_sets(which):
    """name -> (B, R as a numpy array (N,3,3) shared or (B,N,3,3) per sample) for one family case."""
    if which == "singles":        # B = 1, N = 1: the first matrix of every sub-family, and the zero matrix
        out = {}
        for R, names in (fam.inside(), fam.outside()):
            seen = set()
            for k, s in enumerate(names):
                if fam.family(s) not in seen:
                    seen.add(fam.family(s))
                    out[s] = (1, R[k:k + 1])
        return out
    if which == "shared_mixed":   # B = 2, one set of 200: both kinds in flight in a workgroup
        return {which: (2, fam.mixed(200)[0])}
    if which == "per_sample":     # B = 3 x 96: one sample all accepted, one all rejected, one mixed
        return {which: (3, np.stack([fam.inside(96)[0], fam.outside(96)[0], fam.mixed(96)[0]]))}
    if which == "many_samples":   # B = 300 x 2: more samples than CUs, one accepted and one rejected matrix per sample
        return {which: (300, np.stack([fam.inside(300, 8)[0], fam.outside(300, 8)[0]], axis=1))}
    if which == "large_mixed":    # B = 1 x 2000: several hypotheses per slot and workgroup (reference cost of the (2, 1100) case)
        return {which: (1, fam.mixed(2000)[0])}
    raise KeyError(which)


def family_case(ahv, dev, B, R_np, seed):
    """make_case inputs with R replaced."""
    vs, ft, _, W1, W2, b2, _ = make_case(ahv, dev, B, 1, False, seed)
    R = torch.from_numpy(np.ascontiguousarray(R_np)).to(dev)
    gs = torch.from_numpy(np.random.RandomState(seed + 7).standard_normal((B, R.shape[-3])).astype(np.float32)).to(dev)
    return vs, ft, R, W1, W2, b2, gs


def both_backwards(ops, vs, ft, R, W1, W2, b2, gs):
    """(recomputing gradients, saved-pre-activation gradients); the training forward's scores must be the inference ones."""
    want = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    scores, ws = ops.score_hypotheses_train(vs, ft, R, W1, W2, b2)
    plain, _ = ops.score_hypotheses(vs, ft, R, W1, W2, b2)
    assert torch.equal(scores, plain)
    saved = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs, workspace=ws)
    return want, saved


@pytest.mark.parametrize("which", ["singles", "shared_mixed", "per_sample", "many_samples", "large_mixed"])
def test_backward_of_near_and_non_rotations_matches_fp64_autograd(ops, ahv, dev, which):
    """Matrices at the edge of what rmw_rotation_like accepts (8 voxels per scatter instruction) and matrices it rejects
    (one voxel per instruction), alone, side by side in a workgroup and many per slot: the five gradients of the recomputing
    AND of the saved-pre-activation backward against the kink-aware fp64 reference, unchanged GRAD_RTOL; the training forward
    gives the inference scores bit for bit, and the two backwards agree to SAVED_RTOL."""
    for k, (name, (B, R_np)) in enumerate(family_sets(which).items()):
        case = family_case(ahv, dev, B, R_np, 400 + 10 * k + B)
        want, saved = both_backwards(ops, *case)
        ref = KinkReference(*case)
        for tag, got in (("recomputing", want), ("saved", saved)):
            errs, n_amb, combo = ref.errors(got)
            print(name, tag, tuple(case[2].shape), {k_: "%.1e" % v for k_, v in zip(GRAD_NAMES, errs)}, "near-kink pre-activations:", n_amb,
                  "flipped:", combo)
            assert all(torch.isfinite(g).all().item() for g in got)
            assert max(errs) < GRAD_RTOL, (name, tag, errs, n_amb)
        between = [relerr(a, b.double()) for a, b in zip(saved, want)]
        print(name, "saved against recomputing:", ["%.1e" % e for e in between])
        assert max(between) < SAVED_RTOL, (name, between)


@pytest.mark.parametrize("saved", [False, True])
def test_backward_is_additive_over_single_hypothesis_calls(ops, ahv, dev, saved):
    """The five gradients of the mixed set equal the sum of N calls with ONE hypothesis each, added up in fp64 on the host.  A
    single-hypothesis call has one busy slot in one workgroup per sample, so no two hypotheses share an instruction stream or
    an image there: a race between the lanes of a scatter instruction, or between the two slots, shows as a difference --
    without any kink fitting, the arithmetic per hypothesis being the same in both arrangements."""
    R_np = fam.mixed(200)[0]
    vs, ft, R, W1, W2, b2, gs = family_case(ahv, dev, 2, R_np, 431)

    def run(r, g):
        r, g = r.contiguous(), g.contiguous()
        if not saved:
            return ops.score_hypotheses_backward(vs, ft, r, W1, W2, b2, g)
        _, ws = ops.score_hypotheses_train(vs, ft, r, W1, W2, b2)
        return ops.score_hypotheses_backward(vs, ft, r, W1, W2, b2, g, workspace=ws)
    full = run(R, gs)
    total = [torch.zeros(t.shape, dtype=torch.float64) for t in full]
    for n in range(R.shape[0]):
        for acc, part in zip(total, run(R[n:n + 1], gs[:, n:n + 1])):
            acc += part.cpu().double()
    errs = [relerr(f.cpu(), t) for f, t in zip(full, total)]
    print("additivity, saved =", saved, {k: "%.1e" % v for k, v in zip(GRAD_NAMES, errs)})
    assert max(errs) < TWO_CALLS_RTOL, dict(zip(GRAD_NAMES, errs))


def test_backward_of_rejected_matrices_is_reproducible(ops, ahv, dev):
    """Two calls on ``outside`` (footprints that do overlap, 46 % of them by the model) agree to rounding, both backwards."""
    case = family_case(ahv, dev, 2, fam.outside()[0], 433)
    a, sa = both_backwards(ops, *case)
    b, sb = both_backwards(ops, *case)
    for tag, x, y in (("recomputing", a, b), ("saved", sa, sb)):
        errs = [relerr(p, q.double()) for p, q in zip(x, y)]
        print("run to run,", tag, ["%.1e" % e for e in errs])
        assert max(errs) < TWO_CALLS_RTOL, (tag, errs)


def tiny_cfg(n):
    return {"RUN_NAME": "t", "DATA": {"NUM_ROTA": n, "BG": True, "SIZE_THR": 25, "OBJ_SIZE": 256, "ACC_THR": 30,
                                       "VIEW_THR": 90},
            "TRAIN": {"MASK": True, "MASK_RATIO": 0.25, "LR": 1e-4}}


def test_infonce_gradients_match_all_torch_graph(ahv, dev):
    """infoNCE_loss under autograd: loss and parameter / volume gradients equal those of the same loss built from
    stock torch operators (the reference's graph, modules/model_co3d.py:41-61)."""
    import math
    torch.manual_seed(3)
    m = ahv.estimator.EstimatorCo3d(tiny_cfg(48)).to(dev).train()
    g = torch.Generator().manual_seed(4)
    vs = (torch.randn(2, 16, 8, 8, 8, generator=g) * 1.1).to(dev).requires_grad_(True)
    vt = (torch.randn(2, 16, 8, 8, 8, generator=g) * 1.1).to(dev).requires_grad_(True)
    gt = ahv.rotations.random_rotations(2, generator=g).to(dev)
    R = torch.cat([gt[:, None], ahv.rotations.random_rotations(2 * 47, generator=g).to(dev).reshape(2, 47, 3, 3)], dim=1)
    loss = m.infoNCE_loss(vs, vt, R, gt)
    params = list(m.feature_aligner.feature_embedding_2d.parameters())
    got = torch.autograd.grad(loss, [vs, vt] + params)

    W1, W2, b2 = (p.detach().double().requires_grad_(True) for p in m.feature_aligner.head_weights())
    vs64, vt64 = vs.detach().double().requires_grad_(True), vt.detach().double().requires_grad_(True)
    from oracle import torch_ref
    ft = torch_ref.forward_3d2d(vt64, W1, W2, b2)
    sim = ref_scores(vs64, ft, R.double(), W1, W2, b2)
    gs = (torch.sum(R.flatten(2) * gt.reshape(-1, 1, 9), dim=-1).clamp(-1, 3) - 1) / 2
    pos = (180 * torch.arccos(gs) / math.pi <= 30)
    e = torch.exp(sim / 0.1)
    ref_loss = (-torch.log((e * pos).sum(dim=-1) / e.sum(dim=-1).clamp(min=1e-8))).mean()
    ref = torch.autograd.grad(ref_loss, [vs64, vt64, W1, W2, b2])
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    for a, b in zip(got, ref):
        assert relerr(a, b.reshape(a.shape)) < GRAD_RTOL


@pytest.mark.parametrize("tag", ["a", "b"])
def test_infonce_matches_the_reference_run_gradients(ahv, dev, tag):
    """G11 `infonce_grad` (tools/gen_golden.py gen_infonce): the loss, similarities and five gradients the
    REFERENCE's own code produced under autograd (utils.rotate_volume utils.py:113-131 + Feature_Aligner.forward_3d2d
    modules/modules.py:112-124 + the loss lines of modules/model_co3d.py:41-61), per-sample hypothesis sets with the
    GT at index 0.  The mirror's infoNCE_loss (one fused HIP launch forward, the three-kernel HIP backward) must
    give the same loss (1e-5), similarities (1e-4 relative, the forward's contract) and gradients (GRAD_RTOL of
    each tensor's largest entry; reference gradients are fp32 here, so a near-kink pre-activation falls back on
    the kink-aware fp64 comparison)."""
    g = load_golden("infonce_grad")
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)
    B, N = g[tag + "_R"].shape[:2]
    m = ahv.estimator.EstimatorCo3d(tiny_cfg(N)).to(dev).train()
    c1, c2 = m.feature_aligner.feature_embedding_2d[0], m.feature_aligner.feature_embedding_2d[2]
    with torch.no_grad():
        c1.weight.copy_(t("W1").reshape(c1.weight.shape))
        c2.weight.copy_(t("W2").reshape(c2.weight.shape))
        c2.bias.copy_(t("b2"))
    vs, vt = t(tag + "_vol_src").requires_grad_(True), t(tag + "_vol_tgt").requires_grad_(True)
    R, gt = t(tag + "_R"), t(tag + "_gt")
    per_sample = m.infoNCE_loss(vs, vt, R, gt, reduce_mean=False)
    loss = m.infoNCE_loss(vs, vt, R, gt)
    assert abs(loss.item() - float(g[tag + "_loss"])) < 1e-5
    assert np.max(np.abs(per_sample.detach().cpu().numpy() - g[tag + "_loss_per_sample"])) < 1e-5
    sim = ahv.ops.score_hypotheses(vs.detach(), m.feature_aligner.forward_3d2d(vt.detach()).detach(), R,
                                   *[w.detach() for w in m.feature_aligner.head_weights()])[0]
    ref_sim = g[tag + "_sim"]
    assert np.max(np.abs(sim.cpu().numpy() - ref_sim) / np.abs(ref_sim).clip(1e-2)) < 1e-4
    got = torch.autograd.grad(loss, [vs, vt, c1.weight, c2.weight, c2.bias])
    errs = {}
    for a, key in zip(got, ("d_vol_src", "d_vol_tgt", "d_W1", "d_W2", "d_b2")):
        ref = torch.from_numpy(g[tag + "_" + key]).double().to(dev)
        errs[key] = relerr(a.reshape(ref.shape), ref)
    print(tag, {k: "%.1e" % v for k, v in errs.items()})
    assert all(v < GRAD_RTOL for v in errs.values()), errs


def test_training_steps_reduce_the_loss(ahv, dev):
    """training_step (modules/model_co3d.py:71-91) end to end: backbone -> encoder (torch autograd) -> sampled
    rotations with the ground truth as hypothesis 0 -> InfoNCE through the HIP backward -> AdamW."""
    torch.manual_seed(0)
    cfg = tiny_cfg(64)
    cfg["TRAIN"]["LR"] = 3e-4
    m = ahv.estimator.EstimatorCo3d(cfg, feature_extractor=ahv.estimator.PatchifyBackbone(seed=1)).to(dev).train()
    (opt,), (sched,) = m.configure_optimizers()
    g = torch.Generator().manual_seed(1)
    batch = {"image": torch.randn(2, 2, 3, 256, 256, generator=g).to(dev),
             "relative_rotation": ahv.rotations.random_rotations(2, generator=g).to(dev)[:, None]}
    losses = []
    for step in range(6):
        opt.zero_grad()
        loss = m.training_step(batch, step)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and len(m.logged["train_loss"]) == 6
    # every aligner parameter takes part, except bn_down, which the reference constructs but never applies
    assert all(p.grad is not None for k, p in m.feature_aligner.named_parameters() if "bn_down" not in k)
    assert min(losses[3:]) < losses[0], losses   # same pair every step: the loss must come down


def test_backward_many_samples_and_gradient_scales(ops, ahv, dev):
    """More samples than workgroups in y (each workgroup flushes / re-zeroes its volume-gradient image between
    samples), and upstream gradients far from 1 (the dV image is fixed point with a per-sample scale derived on the
    device from max|du|)."""
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 260, 3, True, 21)
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    leaves = [x.double().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
    ref = torch.autograd.grad(ref_scores(leaves[0], leaves[1], R.double(), *leaves[2:]), leaves, grad_outputs=gs.double())
    for a, b in zip(got, ref):
        assert relerr(a, b.reshape(a.shape)) < GRAD_RTOL
    # per-sample check of the volume gradient (a global max would hide a sample that was dropped)
    per = ((got[0].double() - ref[0]).flatten(1).abs().max(dim=1).values / ref[0].flatten(1).abs().max(dim=1).values)
    assert per.max().item() < GRAD_RTOL

    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, 2, 50, False, 22)
    base = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    for scale in (1e-9, 1e7):
        mixed = gs * torch.tensor([[scale], [1.0]], device=dev)       # two samples, very different magnitudes
        out = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, mixed)
        assert relerr(out[0][0], base[0][0].double() * scale) < 1e-5
        assert relerr(out[0][1], base[0][1].double()) < 1e-5
    nan = gs.clone()
    nan[0, 3] = float("nan")                                          # poisoned sample -> NaN, the other one intact
    out = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, nan)
    assert torch.isnan(out[0][0]).any() and torch.isfinite(out[0][1]).all()
    assert relerr(out[0][1], base[0][1].double()) < 1e-5


def test_graphed_train_step_matches_eager(ahv, dev):
    """harness.GraphedTrainStep (whole iteration in one hipGraph) against the eager iteration: same rotations
    (same seed and draw counter), masking off -> same losses and same parameters after three steps."""
    import copy
    cfg = tiny_cfg(48)
    cfg["TRAIN"]["MASK"] = False
    torch.manual_seed(0)
    m1 = ahv.estimator.EstimatorCo3d(cfg, feature_extractor=ahv.estimator.PatchifyBackbone(seed=1)).to(dev).train()
    m2 = copy.deepcopy(m1)
    g = torch.Generator().manual_seed(5)
    batches = [{"image": torch.randn(2, 2, 3, 256, 256, generator=g).to(dev),
                "relative_rotation": ahv.rotations.random_rotations(2, generator=g).to(dev)[:, None]} for _ in range(3)]
    state0 = copy.deepcopy(m2.state_dict())
    step = ahv.harness.GraphedTrainStep(m2, batch_size=2, device=dev, warmup=2)
    # the warm-up iterations trained m2 on zeros: rewind weights, optimizer state and the rotation draw counter
    m2.load_state_dict(state0)
    for st in step.optimizer.state.values():
        for v in st.values():
            if torch.is_tensor(v):
                v.zero_()
    step._draws = 0
    graphed = [float(step(b).item()) for b in batches]

    opt = torch.optim.AdamW([{"params": m1.feature_aligner.parameters(), "lr": 1e-4},
                             {"params": m1.feature_extractor.parameters(), "lr": 1e-4}], eps=1e-5)
    eager = []
    for i, b in enumerate(batches):
        gt = b["relative_rotation"].squeeze(1)
        R = torch.cat([gt[:, None], ahv.ops.random_rotations(2 * 47, seed=torch.initial_seed() + i + 1, device=dev).reshape(2, 47, 3, 3)], dim=1)
        opt.zero_grad()
        vs, vt = m1.feature_aligner.forward_2d3d(m1.feature_extraction(b["image"][:, 0]), m1.feature_extraction(b["image"][:, 1]),
                                                 random_mask=False, mask_ratio=0.0)
        loss = m1.infoNCE_loss(vs, vt, R, gt, reduce_mean=True)
        loss.backward()
        opt.step()
        eager.append(float(loss.item()))
    assert np.allclose(graphed, eager, rtol=2e-4, atol=1e-5), (graphed, eager)
    # Adam's first steps are +-lr * sign-like, so rounding-level gradient differences (other GEMM backend, float
    # atomics) move single weights by a fraction of lr: compare the UPDATE vectors, not the weights elementwise
    up1 = torch.cat([(a - state0[k]).flatten() for k, a in m1.state_dict().items() if a.is_floating_point()])
    up2 = torch.cat([(b - state0[k]).flatten() for k, b in m2.state_dict().items() if b.is_floating_point()])
    cos = torch.nn.functional.cosine_similarity(up1, up2, dim=0).item()
    assert cos > 0.999 and up1.abs().max().item() > 1e-5, cos
    assert (up1 - up2).abs().max().item() < 6e-4


def test_backward_at_the_co3d_training_size(ops, ahv, dev):
    """The reference's CO3D training size (train_estimator_co3d.py:12-15: NUM_ROTA = 9000, BS = 32; per-sample
    rotation sets, modules/model_co3d.py:41-61): 288 000 hypotheses forward + backward in one call.
      * workspace = the size the ABI reports (2.36 GB: 8 KiB of dL/du per hypothesis);
      * a 2 x 1100 sub-problem EMBEDDED in the batch (samples 5 and 17, hypotheses 3000..4099; dL/dscore = 0
        everywhere else) meets the kink-aware fp64 reference, and samples without upstream gradient get exact zeros;
      * with dL/dscore on all 288 000 hypotheses the gradients are finite and ADDITIVE over a split of the hypothesis
        axis (the 64-bit fixed-point image of dV and its per-sample headroom guard at 9000 hypotheses per sample)."""
    B, N = 32, 9000
    lib = ahv._lib.load()
    cu = lib.ahv_device_cu_count()
    # dL/du (8 KiB per hypothesis) + max|du| per sample (padded to 4 words) + one dW1 partial per workgroup
    assert lib.ahv_score_hypotheses_backward_workspace_bytes(B, N) == 4 * (2048 * B * N + ((B + 3) & ~3) + cu * 32 * 384)
    vs, ft, R, W1, W2, b2, gs = make_case(ahv, dev, B, N, True, 77)
    sub_b, lo, hi = [5, 17], 3000, 4100
    gsub = torch.zeros_like(gs)
    for b in sub_b:
        gsub[b, lo:hi] = gs[b, lo:hi]
    got = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gsub)
    others = [b for b in range(B) if b not in sub_b]
    assert got[0][others].abs().max().item() == 0.0 and got[1][others].abs().max().item() == 0.0
    sub = (got[0][sub_b], got[1][sub_b], got[2], got[3], got[4])
    errs, n_amb, combo = kink_aware_errors(sub, vs[sub_b], ft[sub_b], R[sub_b][:, lo:hi].contiguous(), W1, W2, b2,
                                           gs[sub_b][:, lo:hi].contiguous())
    print("embedded 2 x 1100:", ["%.1e" % e for e in errs], "near-kink:", n_amb, "flipped:", combo)
    assert max(errs) < GRAD_RTOL, (errs, n_amb)
    # every hypothesis carries gradient: finite, and the sum of the two half-batches of hypotheses
    full = ops.score_hypotheses_backward(vs, ft, R, W1, W2, b2, gs)
    assert all(torch.isfinite(g).all().item() for g in full)
    half = N // 2
    ga = ops.score_hypotheses_backward(vs, ft, R[:, :half].contiguous(), W1, W2, b2, gs[:, :half].contiguous())
    gb = ops.score_hypotheses_backward(vs, ft, R[:, half:].contiguous(), W1, W2, b2, gs[:, half:].contiguous())
    for name, f, a, b_ in zip(["vol_src", "feat_tgt", "W1", "W2", "b2"], full, ga, gb):
        err = relerr(f, (a.double() + b_.double()))
        assert err < 2e-5, (name, err)     # fp32 accumulation order differs between one pass and two
