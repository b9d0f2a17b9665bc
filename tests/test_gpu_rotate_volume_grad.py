"""The rotation gradient of the op-level rotate_volume (ahv_rotate_volume_rotation_grad_f32, ops.rotate_volume_rotation_grad,
ops.rotate_volume_autograd) against torch autograd in fp64 on the CPU through oracle/torch_ref.py's rotate_volume
(tests/rotate_grad_reference.py has the reference, the error measure and the rule for ambiguous hypotheses).

The yardstick is what stock torch in fp32 on the CPU reaches against fp64 on THESE cases (``python -m
tests.test_gpu_rotate_volume_grad`` re-measures it and the ambiguous shares, no GPU needed).  Measured: maximum 2.43e-6 (the
130-hypothesis case, seed 403), median 5e-7, 6.3e-7 on the edge set with grad_out from EDGE_SEED; 3 of the 1 024 hypotheses of the seed-404 case are
ambiguous and none of any other case.  The bar is 10 x that maximum -- margin for a different summation order -- and never
looser than the project's GRAD_RTOL = 2e-4: PARITY_BAR = 2.43e-5."""
import types

import numpy as np
import pytest
import torch

from . import rotate_grad_reference as rg
from .conftest import load_golden

pytestmark = pytest.mark.gpu
FP32_CPU_MAX = 2.43e-6                      # measured, see above
PARITY_BAR = min(10 * FP32_CPU_MAX, 2e-4)
EDGE_SEED = 408
# (N, C, D, H, W, shared volume?, seed)
CASES = [(1, 16, 8, 8, 8, True, 400),       # a lone hypothesis
         (37, 16, 8, 8, 8, True, 401),
         (9, 16, 8, 8, 8, False, 402),
         (130, 16, 8, 8, 8, False, 403),    # per-sample volumes, re-staged per hypothesis
         (1024, 16, 8, 8, 8, True, 404),    # more hypotheses than workgroups: the grid-stride loop runs
         (33, 3, 4, 6, 5, False, 405),      # the generic kernel
         (17, 5, 2, 3, 9, True, 406),       # unequal axes: each S_a is distinct
         (64, 1, 8, 8, 8, True, 407)]       # 8^3 but not 16 channels: must take the generic kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def edge_case():
    """The edge_rotations set on score_n128's vol_src with a seeded grad_out."""
    g, e = load_golden("score_n128"), load_golden("edge_rotations")
    R = torch.from_numpy(np.ascontiguousarray(e["R"]))
    vol = torch.from_numpy(np.ascontiguousarray(g["vol_src"]))[0]
    return (vol[None].expand(R.shape[0], -1, -1, -1, -1), R, rg.seeded_grad_out(EDGE_SEED, R.shape[0])), [str(n) for n in e["names"]]


def all_cases(pkg):
    for N, C, D, H, W, shared, seed in CASES:
        yield ("N%d_%dx%dx%dx%d_%s" % (N, C, D, H, W, "shared" if shared else "per"),
               rg.random_case(pkg.rotations.haar_rotations_np, N, C, D, H, W, shared, seed), None)
    case, names = edge_case()
    yield "edge_rotations", case, names


def case_by_n(ahv, n):
    (row,) = [c for c in CASES if c[0] == n]
    return rg.random_case(ahv.rotations.haar_rotations_np, *row)


def on(dev, vol, R, g):
    """The case on the device; a shared volume stays a stride-0 expand of one."""
    if vol.stride(0) == 0 and vol.shape[0] > 1:
        vol = vol[0].to(dev)[None].expand(vol.shape[0], -1, -1, -1, -1)
    else:
        vol = vol.to(dev)
    return vol, R.to(dev), g.to(dev)


@pytest.mark.parametrize("k", range(len(CASES) + 1))
def test_parity_with_fp64_autograd(ahv, ops, dev, k):
    name, (vol, R, g), names = list(all_cases(ahv))[k]
    ref = rg.ref_rotate_grad(vol, R, g)
    amb = rg.ambiguous(R, *vol.shape[2:])
    left = rg.check_ambiguous(name, amb, names)
    got = ops.rotate_volume_rotation_grad(*on(dev, vol, R, g))
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32
    err = rg.hyp_err(got, ref)
    worst = err[~amb].max().item()
    print("%s: %d hypotheses, %d ambiguous, max err %.3g (median %.3g), all %.3g, bar %.3g"
          % (name, amb.numel(), left, worst, err[~amb].median().item(), err.max().item(), PARITY_BAR))
    assert torch.isfinite(got).all()
    assert worst <= PARITY_BAR, (name, worst)


def test_bitwise_reproducible(ahv, ops, dev):
    """The nine numbers of a hypothesis do not depend on the run, on N, on the grid or on the cut into calls."""
    vol, R, g = on(dev, *case_by_n(ahv, 130))
    f = ops.rotate_volume_rotation_grad
    whole = f(vol, R, g)
    assert torch.equal(whole, f(vol, R, g))
    parts = [f(vol[a:b], R[a:b], g[a:b]) for a, b in ((0, 1), (1, 65), (65, 130))]
    assert torch.equal(whole, torch.cat(parts))
    vol, R, g = on(dev, *case_by_n(ahv, 1024))
    assert vol.stride(0) == 0
    assert torch.equal(f(vol, R, g)[:37], f(vol[:37], R[:37], g[:37]))


@pytest.mark.parametrize("n", [37, 130, 17])
def test_autograd_edge(ahv, ops, dev, n):
    vol, R, g = on(dev, *case_by_n(ahv, n))
    shared = vol.stride(0) == 0
    want = ops.rotate_volume_rotation_grad(vol, R, g)
    # R alone requires grad
    Rl = R.clone().requires_grad_(True)
    out = ops.rotate_volume_autograd(vol, Rl)
    assert out.requires_grad and torch.equal(out, ops.rotate_volume(vol, R))
    out.backward(g)
    assert torch.equal(Rl.grad, want)
    assert vol.grad is None
    # the volume alone: today's adjoint
    base = (vol[0] if shared else vol).clone().requires_grad_(True)
    ops.rotate_volume_autograd(base[None].expand(n, -1, -1, -1, -1) if shared else base, R).backward(g)
    plain = base.grad
    # both
    base = (vol[0] if shared else vol).clone().requires_grad_(True)
    Rl = R.clone().requires_grad_(True)
    ops.rotate_volume_autograd(base[None].expand(n, -1, -1, -1, -1) if shared else base, Rl).backward(g)
    assert torch.equal(Rl.grad, want)
    assert base.grad.shape == base.shape and plain.shape == base.shape    # the shared form: the base's gradient
    # float atomics: rounding, not bits (the bar of tests/test_gpu_boundary.py for this adjoint)
    assert ((base.grad.double() - plain.double()).abs().max() / plain.double().abs().max()).item() < 1e-5
    with torch.no_grad():
        out = ops.rotate_volume_autograd(vol, R.clone().requires_grad_(True))
    assert not out.requires_grad and out.grad_fn is None


def test_non_finite_rotation(ahv, ops, dev):
    for n in (130, 33):   # both kernels
        vol, R, g = on(dev, *case_by_n(ahv, n))
        want = ops.rotate_volume_rotation_grad(vol, R, g)
        bad = R.clone()
        bad[3, 1, 2] = float("nan")
        bad[7, 0, 0] = float("inf")
        got = ops.rotate_volume_rotation_grad(vol, bad, g)
        hit = torch.zeros(n, dtype=torch.bool, device=dev)
        hit[3] = hit[7] = True
        assert torch.isnan(got[hit]).all()
        assert torch.equal(got[~hit], want[~hit])


@pytest.fixture
def patched(ahv):
    """patch.install() on a stand-in ``utils``; patch.calls is left with the keys it had (the counter of this path appears
    with its first call, and other tests compare the whole dict)."""
    um, mm = types.ModuleType("utils"), types.ModuleType("modules.modules")
    um.rotate_volume = lambda *a, **k: None

    class Feature_Aligner(torch.nn.Module):  # noqa: N801
        def forward_3d2d(self, x):
            raise AssertionError("not used")
    mm.Feature_Aligner = Feature_Aligner
    had = "rotate_volume_autograd" in ahv.patch.calls
    ahv.patch.install(um, mm)
    try:
        yield um
    finally:
        ahv.patch.uninstall()
        if not had:
            ahv.patch.calls.pop("rotate_volume_autograd", None)


def test_drop_in_back_propagates_into_the_rotations(ahv, ops, dev, patched):
    vol, R, g = on(dev, *case_by_n(ahv, 37))
    want = ops.rotate_volume_rotation_grad(vol, R, g)
    Rl = R.clone().requires_grad_(True)
    n0 = ahv.patch.calls.get("rotate_volume_autograd", 0)
    k0 = ahv.patch.calls["rotate_volume_kernel"]
    out = patched.rotate_volume(vol, Rl)
    assert type(out) is torch.Tensor and out.requires_grad
    assert ahv.patch.calls["rotate_volume_autograd"] == n0 + 1 and ahv.patch.calls["rotate_volume_kernel"] == k0
    (out * g).sum().backward()        # a loss of the caller's own on the voxels
    assert torch.equal(Rl.grad, want)
    with pytest.raises(NotImplementedError, match="score_hypotheses"):
        ops.rotate_volume(vol, R.clone().requires_grad_(True))


if __name__ == "__main__":   # the fp32-on-CPU yardstick and the ambiguous shares of the cases above (no GPU)
    import importlib
    pkg = importlib.import_module("3dahv_amd")
    top = 0.0
    for name, (vol, R, g), names in all_cases(pkg):
        ref = rg.ref_rotate_grad(vol, R, g)
        f32 = rg.ref_rotate_grad(vol, R, g, dtype=torch.float32)
        amb = rg.ambiguous(R, *vol.shape[2:])
        left = rg.check_ambiguous(name, amb, names)
        err = rg.hyp_err(f32, ref)
        top = max(top, err[~amb].max().item())
        print("%-24s %5d hypotheses, %3d ambiguous %s; torch fp32: median %.2g max %.3g (ambiguous included: %.3g)"
              % (name, amb.numel(), left, [names[j] for j in torch.nonzero(amb).flatten().tolist()] if names else "",
                 err[~amb].median().item(), err[~amb].max().item(), err.max().item()))
    print("maximum over the unambiguous hypotheses: %.3g" % top)
