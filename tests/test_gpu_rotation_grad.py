"""d score / d R (ahv_score_rotation_grad_f32) against torch autograd in fp64 on the CPU through the reference's op
sequence (oracle/torch_ref.py) with ``R.requires_grad_()``.

Error per hypothesis: max|got - ref| / max|ref| over its nine entries.  The yardstick is what stock torch in fp32 on the CPU
reaches against fp64 on THESE cases (``python -m tests.test_gpu_rotation_grad`` re-measures it, no GPU needed); measured:
median 6e-7 and maximum 2.5e-6 over the unambiguous hypotheses of all cases below (the maximum is in (1,1024,F); the edge
set reaches 1.3e-6).  The bar is 10 x that maximum -- margin for a different summation order, fp32 MFMA chains of 384
against ATen's -- and never looser than the project's GRAD_RTOL = 2e-4: PARITY_BAR = 2.5e-5.

A hypothesis is ambiguous, and left out, when the fp64 reference finds a pre-activation with 0 < |u| < KINK_TAU = 2e-6 or a
sample coordinate with 0 < |i - round(i)| < 2e-6.  An exactly integer coordinate is NOT ambiguous (grid_sampler_3d_backward's
convention decides it), and neither is a pre-activation of exactly 0 (a position all of whose samples fall outside the
volume, as under 2 I: F.relu's sub-gradient there is 0, the kernel's ``u > 0`` mask says the same).  At most 5 % of a case
may be left out (none of a case with fewer than 20 hypotheses), never identity, a cube rotation, 0.5 I or 2 I; the
axis-aligned 45-degree turns may fall out and are not counted.  check_ambiguous enforces these caps on every case, in the
GPU test and in the CPU command above alike; the seeds in CASES / FAMILY_CASES were picked with that command so that they
hold ((2,9,T) runs on seed 331: seed 330 leaves one of its 18 hypotheses out, which is over the cap of a small case).

The two ``families_*`` cases put the matrices of tests/rotation_families.py through the kernel (B = 2, shared set): what the dV
scatter's classifier accepts up to its threshold together with the full-rank matrices it rejects (scaled, sheared,
non-orthonormal: 400 hypotheses), and the rank-deficient ones -- projections of rank 2 and 1, the zero matrix -- as a
case of their own (128 hypotheses; their ambiguous share is under the cap, so they stay in).  The yardstick re-measured on
them: 2.1e-6 and 1.3e-6, below the 2.5e-6 of (1,1024,F) -- PARITY_BAR is unchanged."""
import numpy as np
import pytest
import torch

from . import rotation_families as fam
from .conftest import load_golden

pytestmark = pytest.mark.gpu
KINK_TAU = 2e-6
FP32_CPU_MAX = 2.5e-6                       # measured, see above
PARITY_BAR = min(10 * FP32_CPU_MAX, 2e-4)
# (B, N, per_sample, seed): seeds kept for which the ambiguous share below holds (measured on the CPU, see the docstring)
CASES = [(1, 1, False, 300), (1, 37, False, 330), (2, 9, True, 331), (3, 130, True, 330), (300, 2, True, 340), (1, 1024, False, 350)]

# (name, full rank?, seed): B = 2 on a shared set of tests/rotation_families.py, see family_case
FAMILY_CASES = [("families_full_rank", True, 360), ("families_rank_deficient", False, 360)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def ref_rotation_grad(vs, ft, R, W1, W2, b2, gs=None, dtype=torch.float64, chunk=128, scale=1.0):
    """(grad_R (B,N,3,3), ambiguous (B,N) bool) by torch autograd on the CPU in ``dtype``.  ``scale``: the magnitude of the case's
    pre-activations relative to the ~1 that KINK_TAU is stated for (tests/backward_cases.py)."""
    from oracle import torch_ref
    import torch.nn.functional as F
    vs, ft, R, W1, W2, b2 = (t.detach().cpu().to(dtype) for t in (vs, ft, R, W1, W2, b2))
    B = vs.shape[0]
    N = R.shape[-3]
    gs = torch.ones(B, N, dtype=dtype) if gs is None else gs.detach().cpu().to(dtype)
    c = (2 * torch.arange(8, dtype=dtype) + 1) / 2 - 4          # 4 * voxel-centre coordinate
    P = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3).flip(-1)   # rows (x_w, y_h, z_d)
    grad = torch.zeros(B, N, 3, 3, dtype=dtype)
    amb = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        for n0 in range(0, N, chunk):
            Rb = (R[b] if R.dim() == 4 else R)[n0:n0 + chunk].clone().requires_grad_(True)
            n = Rb.shape[0]
            vol = torch_ref.rotate_volume(vs[b][None].expand(n, -1, -1, -1, -1), Rb)
            m, ch, d, h, w = vol.shape
            slabs = torch.cat([vol.permute(0, 1, 4, 2, 3).reshape(m, ch * w, d, h), vol.permute(0, 1, 3, 2, 4).reshape(m, ch * h, d, w),
                               vol.reshape(m, ch * d, h, w)], dim=1)                   # modules/modules.py:115-118
            u = F.conv2d(slabs, W1.reshape(32, 384, 1, 1))
            v = F.conv2d(F.relu(u), W2.reshape(32, 32, 1, 1), b2)
            f = F.normalize(v, p=2, dim=1).flatten(2)
            s = (f * ft[b][None]).sum(dim=1).mean(dim=-1)
            (g,) = torch.autograd.grad(s, Rb, grad_outputs=gs[b, n0:n0 + n])
            grad[b, n0:n0 + n] = g
            i = torch.einsum("nab,pb->npa", Rb.detach(), P) + 3.5
            frac = (i - i.round()).abs()
            amb[b, n0:n0 + n] = ((u.detach().abs() < KINK_TAU * scale) & (u.detach() != 0)).flatten(1).any(dim=1) | ((frac > 0) & (frac < KINK_TAU)).flatten(1).any(dim=1)
    return grad, amb


def hyp_err(got, ref):
    """(B,N) max|got - ref| / max|ref| over the nine entries of each hypothesis."""
    d = (got.detach().cpu().double() - ref.double()).abs().flatten(2).max(dim=2).values
    return d / ref.double().abs().flatten(2).max(dim=2).values.clamp_min(1e-30)


def make_case(ahv, B, N, per_sample, seed):
    g = load_golden("score_n128")
    rng = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    vs = t((rng.standard_normal((B, 16, 8, 8, 8)) * 1.1).astype(np.float32))
    ft = torch.nn.functional.normalize(t(rng.standard_normal((B, 32, 64)).astype(np.float32)), dim=1)
    R = ahv.rotations.haar_rotations_np(N * (B if per_sample else 1), seed + 1)
    R = t(R.reshape(B, N, 3, 3) if per_sample else R)
    gs = t(rng.standard_normal((B, N)).astype(np.float32))
    return vs, ft, R, t(g["W1"]), t(g["W2"]), t(g["b2"]), gs


def edge_case():
    """The score_n128 pair (target features by stock torch in fp32) with the edge_rotations set."""
    from oracle import torch_ref
    g, e = load_golden("score_n128"), load_golden("edge_rotations")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    W1, W2, b2 = t(g["W1"]), t(g["W2"]), t(g["b2"])
    with torch.no_grad():
        ft = torch_ref.forward_3d2d(t(g["vol_tgt"]), W1, W2, b2).contiguous()
    return (t(g["vol_src"]), ft, t(e["R"]), W1, W2, b2, None), [str(n) for n in e["names"]]


def family_case(ahv, full_rank, seed):
    """B = 2, one shared set from tests/rotation_families.py on make_case's inputs: ``inside`` (what the dV scatter's
    classifier accepts, up to its threshold) plus the full-rank members of ``outside``, or the rank-deficient members of
    ``outside`` (projections of rank 2 and 1, the zero matrix) on their own."""
    (Ri, _), (Ro, no) = fam.inside(), fam.outside()
    pick = [k for k, s in enumerate(no) if fam.is_full_rank(s) == full_rank]
    R = np.concatenate([Ri, Ro[pick]]) if full_rank else Ro[pick]
    vs, ft, _, W1, W2, b2, _ = make_case(ahv, 2, 1, False, seed)
    gs = torch.from_numpy(np.random.RandomState(seed + 7).standard_normal((2, R.shape[0])).astype(np.float32))
    return vs, ft, torch.from_numpy(np.ascontiguousarray(R)), W1, W2, b2, gs


def all_cases(ahv):
    for B, N, per, seed in CASES:
        yield "B%d_N%d_%s" % (B, N, "per" if per else "shared"), make_case(ahv, B, N, per, seed), None
    case, names = edge_case()
    yield "edge_rotations", case, names
    for tag, full_rank, seed in FAMILY_CASES:
        yield tag, family_case(ahv, full_rank, seed), None


def check_ambiguous(name, amb, names):
    n = amb.numel()
    left = int(amb.sum())
    counted = left
    if names is not None:
        for j in torch.nonzero(amb[0]).flatten().tolist():
            assert not (names[j] in ("identity", "half", "double") or names[j].startswith("cube")), names[j]
            if names[j] in ("x45", "y45", "z45"):   # may legitimately fall out (docstring): not counted against the 5 %
                counted -= 1
    assert counted <= (0.05 * n if n >= 20 else 0), "%s: %d of %d hypotheses ambiguous" % (name, left, n)
    return left


@pytest.mark.parametrize("k", range(len(CASES) + 1 + len(FAMILY_CASES)))
def test_parity_with_fp64_autograd(ahv, ops, dev, k):
    name, case, names = list(all_cases(ahv))[k]
    vs, ft, R, W1, W2, b2, gs = case
    ref, amb = ref_rotation_grad(vs, ft, R, W1, W2, b2, gs)
    left = check_ambiguous(name, amb, names)
    d = lambda x: None if x is None else x.to(dev)
    got = ops.score_rotation_grad(d(vs), d(ft), d(R), d(W1), d(W2), d(b2), d(gs))
    assert tuple(got.shape) == tuple(ref.shape)
    err = hyp_err(got, ref)
    keep = ~amb
    worst = err[keep].max().item()
    print("%s: %d hypotheses, %d ambiguous, max err %.3g (median %.3g), all %.3g, bar %.3g"
          % (name, amb.numel(), left, worst, err[keep].median().item(), err.max().item(), PARITY_BAR))
    assert torch.isfinite(got).all()
    assert worst <= PARITY_BAR, (name, worst)


def golden_case():
    """tests/golden/rotation_grad.npz (tools/gen_golden.py gen_rotation_grad): the inputs of score_n128, its first 32 rotations
    and the edge set; grad_R by the REFERENCE's own utils.rotate_volume + Feature_Aligner.forward_3d2d under torch autograd,
    as shipped (fp32) and cast to fp64.  Returns (case with the reference's fp32 target features, names, golden)."""
    g, r = load_golden("score_n128"), load_golden("rotation_grad")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return (t(g["vol_src"]), t(g["f_tgt"]), t(r["R"]), t(g["W1"]), t(g["W2"]), t(g["b2"]), None), [str(n) for n in r["names"]], r


def test_parity_with_the_reference_golden(ahv, ops, dev):
    """The kernel against the gradient the reference's own code produced (fp64 run), same error measure and bar; the
    ambiguous hypotheses are found with the fp64 restatement (tests/test_rotation_grad_golden_cpu.py pins that the
    restatement's gradient IS the file's)."""
    case, names, gold = golden_case()
    vs, ft, R, W1, W2, b2, _ = case
    _, amb = ref_rotation_grad(vs, ft, R, W1, W2, b2)
    left = check_ambiguous("golden", amb, names)
    got = ops.score_rotation_grad(*(x.to(dev) for x in (vs, ft, R, W1, W2, b2)))
    err = hyp_err(got, torch.from_numpy(gold["grad_R_f64"])[None])
    worst = err[~amb].max().item()
    print("golden: %d hypotheses, %d ambiguous, max err %.3g (median %.3g), bar %.3g"
          % (amb.numel(), left, worst, err[~amb].median().item(), PARITY_BAR))
    assert torch.isfinite(got).all()
    assert worst <= PARITY_BAR, worst


def test_bitwise_invariant(ahv, ops, dev):
    """grad_R[b][n] does not depend on N, on the cut into calls, on a shared / per-sample set, on B or on grad_scores = None."""
    vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in make_case(ahv, 3, 1100, False, 77))
    f = lambda v, t, r, g=None: ops.score_rotation_grad(v, t, r, W1, W2, b2, g)
    whole = f(vs, ft, R, gs)
    parts = torch.cat([f(vs, ft, R[:300], gs[:, :300].contiguous()), f(vs, ft, R[300:], gs[:, 300:].contiguous())], dim=1)
    assert torch.equal(whole, parts)
    assert torch.equal(whole, f(vs, ft, R[None].expand(3, -1, -1, -1).contiguous(), gs))
    for b in range(3):
        assert torch.equal(whole[b:b + 1], f(vs[b:b + 1], ft[b:b + 1], R, gs[b:b + 1]))
    assert torch.equal(f(vs, ft, R), f(vs, ft, R, torch.ones_like(gs)))
    assert torch.equal(f(vs, ft, R[:1], gs[:, :1].contiguous()), whole[:, :1])


def test_autograd_edge(ahv, ops, dev):
    for per in (False, True):
        vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in make_case(ahv, 2, 50, per, 91))
        want = ops.score_rotation_grad(vs, ft, R, W1, W2, b2, gs)
        want = want if per else want.sum(dim=0)

        def run(r_needs):
            leaves = [x.clone().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
            Rl = R.clone().requires_grad_(r_needs)
            s = ops.score_hypotheses_autograd(leaves[0], leaves[1], Rl, *leaves[2:])
            s.backward(gs)
            return Rl.grad, [x.grad for x in leaves]
        gR, others = run(True)
        none, plain = run(False)
        assert none is None
        assert torch.equal(gR, want)
        for a, b in zip(others, plain):   # sums over 100 hypotheses by float atomics: the order of the terms is the hardware's
            assert torch.allclose(a, b, rtol=0, atol=2e-4 * b.abs().max().item())
        # R alone requires grad: nothing is detached silently, and only the rotation kernel runs
        Rl = R.clone().requires_grad_(True)
        s, _ = ops.score_hypotheses(vs, ft, Rl, W1, W2, b2)
        assert s.requires_grad
        s.backward(gs)
        assert torch.equal(Rl.grad, want)
        with pytest.raises(RuntimeError, match="no autograd edge"):
            ops.verify_pair(vs, vs, R.clone().requires_grad_(True), W1, W2, b2)
        with pytest.raises(NotImplementedError, match="score_hypotheses"):
            ops.rotate_volume(vs[:1], R.reshape(-1, 3, 3)[:1].clone().requires_grad_(True))


def test_other_gradients_keep_their_bits(ahv, ops, dev):
    """The five other gradients are the same bits whether or not R requires grad.  They are accumulated with float atomics
    (include/ahv.h: reproducible to rounding, not bitwise), so two runs can only be compared bit for bit where no more than
    two terms meet in a word -- a + b is commutative, a sum of three is not associative: B = 1, N = 2 (one workgroup per
    kernel, one hypothesis per wave).  test_autograd_edge compares the larger cases to rounding."""
    vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in make_case(ahv, 1, 2, False, 93))

    def run(r_needs):
        leaves = [x.clone().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
        Rl = R.clone().requires_grad_(r_needs)
        ops.score_hypotheses_autograd(leaves[0], leaves[1], Rl, *leaves[2:]).backward(gs)
        return [x.grad for x in leaves]
    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def test_non_finite_rotation(ahv, ops, dev):
    """A NaN / inf entry of R: NaN for that hypothesis (as autograd), the others keep their bits; the ascent step leaves
    such a seed where it is."""
    vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in make_case(ahv, 2, 12, True, 57))
    want = ops.score_rotation_grad(vs, ft, R, W1, W2, b2, gs)
    bad = R.clone()
    bad[0, 3, 1, 2] = float("nan")
    bad[1, 7, 0, 0] = float("inf")
    got = ops.score_rotation_grad(vs, ft, bad, W1, W2, b2, gs)
    hit = torch.zeros(2, 12, dtype=torch.bool, device=dev)
    hit[0, 3] = hit[1, 7] = True
    assert torch.isnan(got[hit]).all()
    assert torch.equal(got[~hit], want[~hit])
    theta = torch.full((2, 12), 0.03, device=dev)
    cand = ops.so3_ascent_candidates(R, got, theta, (0.5, 1.0)).reshape(2, 12, 3, 3, 3)
    assert torch.equal(cand[0, 3], R[0, 3].expand(3, 3, 3)) and torch.equal(cand[1, 7], R[1, 7].expand(3, 3, 3))


def test_non_finite_sample(ahv, ops, dev):
    vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in make_case(ahv, 3, 40, False, 55))
    bad = vs.clone()
    bad[1, 5, 3, 4, 2] = float("nan")
    got = ops.score_rotation_grad(bad, ft, R, W1, W2, b2, gs)
    assert torch.isnan(got[1]).all()
    for b in (0, 2):
        assert torch.isfinite(got[b]).all()
        assert torch.equal(got[b:b + 1], ops.score_rotation_grad(vs[b:b + 1], ft[b:b + 1], R, W1, W2, b2, gs[b:b + 1]))


if __name__ == "__main__":   # the fp32-on-CPU yardstick and the ambiguous shares of the cases above (no GPU)
    import importlib
    pkg = importlib.import_module("3dahv_amd")
    top = 0.0
    for name, case, names in all_cases(pkg):
        ref, amb = ref_rotation_grad(*case)
        f32, _ = ref_rotation_grad(*case, dtype=torch.float32)
        left = check_ambiguous(name, amb, names)
        err = hyp_err(f32, ref)
        top = max(top, err[~amb].max().item())
        print("%-22s %5d hypotheses, %3d ambiguous %s; torch fp32: median %.2g max %.2g (ambiguous included: %.2g)"
              % (name, amb.numel(), left, [names[j] for j in torch.nonzero(amb[0]).flatten().tolist()] if names else "",
                 err[~amb].median().item(), err[~amb].max().item(), err.max().item()))
    print("maximum over the unambiguous hypotheses: %.3g" % top)
