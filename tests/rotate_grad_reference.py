"""Reference for the rotation gradient of the op-level rotate_volume (ahv_rotate_volume_rotation_grad_f32): torch autograd on
the CPU through oracle/torch_ref.py's rotate_volume (F.affine_grid + F.grid_sample, the reference's utils.py:113-131) with
``R.requires_grad_()``.  Shared by tests/test_gpu_rotate_volume_grad.py and tests/test_rotate_volume_grad_cpu.py; no test here.

Error per hypothesis: max|got - ref| / max|ref| over its nine entries.  A hypothesis is ambiguous when some sample coordinate
has 0 < |i - round(i)| < KINK_TAU = 2e-6 (the value of tests/test_gpu_rotation_grad.py, without that file's ReLU clause:
there is no head here).  An exactly integer coordinate is NOT ambiguous: grid_sampler_3d_backward's convention decides it."""
import numpy as np
import torch

KINK_TAU = 2e-6
# never left out as ambiguous (beside every cube rotation)
PINNED = ("identity", "half", "double", "zero")


def ref_rotate_grad(volume, R, grad_out, dtype=torch.float64, chunk=256):
    """grad_R (N,3,3) of <grad_out, rotate_volume(volume, R)> by torch autograd on the CPU in ``dtype``.  ``volume`` is
    (N,C,D,H,W) -- a stride-0 expand stays one -- or one (C,D,H,W) volume shared by all N."""
    from oracle import torch_ref
    volume, R, grad_out = (t.detach().cpu().to(dtype) for t in (volume, R, grad_out))
    N = R.shape[0]
    if volume.dim() == 4:
        volume = volume[None].expand(N, -1, -1, -1, -1)
    out = torch.zeros(N, 3, 3, dtype=dtype)
    for n0 in range(0, N, chunk):
        Rc = R[n0:n0 + chunk].clone().requires_grad_(True)
        rot = torch_ref.rotate_volume(volume[n0:n0 + chunk], Rc)
        (g,) = torch.autograd.grad(rot, Rc, grad_outputs=grad_out[n0:n0 + chunk])
        out[n0:n0 + chunk] = g
    return out


def ambiguous(R, D, H, W):
    """(N,) bool: some sample coordinate of the hypothesis lies within KINK_TAU of an integer without being one (fp64)."""
    R = R.detach().cpu().double()
    ax = lambda s: (2 * torch.arange(s, dtype=torch.float64) + 1) / s - 1
    z, y, x = torch.meshgrid(ax(D), ax(H), ax(W), indexing="ij")
    P = torch.stack([x, y, z], dim=-1).reshape(-1, 3)                     # rows (x_w, y_h, z_d)
    S = torch.tensor([W, H, D], dtype=torch.float64)
    i = ((torch.einsum("nab,pb->npa", R, P) + 1) * S - 1) / 2
    frac = (i - i.round()).abs()
    return ((frac > 0) & (frac < KINK_TAU)).flatten(1).any(dim=1)


def hyp_err(got, ref):
    """(N,) max|got - ref| / max|ref| over the nine entries of each hypothesis."""
    d = (got.detach().cpu().double() - ref.double()).abs().flatten(1).max(dim=1).values
    return d / ref.double().abs().flatten(1).max(dim=1).values.clamp_min(1e-30)


def check_ambiguous(name, amb, names=None):
    """The caps on what may be left out: at most 5 % of a case, none of a case under 20 hypotheses, never identity, a cube
    rotation, half, double or zero.  Returns the number left out."""
    n, left = amb.numel(), int(amb.sum())
    if names is not None:
        for j in torch.nonzero(amb).flatten().tolist():
            assert not (names[j] in PINNED or names[j].startswith("cube")), names[j]
    assert left <= (0.05 * n if n >= 20 else 0), "%s: %d of %d hypotheses ambiguous" % (name, left, n)
    return left


def random_case(haar, N, C, D, H, W, shared, seed):
    """(volume, R, grad_out) of a row of the GPU test's table: volume = standard_normal * 1.1 from RandomState(seed) -- one
    (C,D,H,W) volume expanded over N when ``shared`` --, R = haar(N, seed + 1), grad_out the next standard_normal draw."""
    rng = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    vol = t((rng.standard_normal((C, D, H, W) if shared else (N, C, D, H, W)) * 1.1).astype(np.float32))
    if shared:
        vol = vol[None].expand(N, -1, -1, -1, -1)
    R = t(haar(N, seed + 1))
    g = t(rng.standard_normal((N, C, D, H, W)).astype(np.float32))
    return vol, R, g


def seeded_grad_out(seed, N, shape=(16, 8, 8, 8)):
    """The upstream gradient of the golden and edge cases: RandomState(seed).standard_normal((N,) + shape) as fp32."""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((N,) + tuple(shape)).astype(np.float32))
