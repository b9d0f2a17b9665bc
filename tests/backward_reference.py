"""The fp64 reference of the fused scorer's backward and its tolerance, shared by tests/test_gpu_backward.py and the C ABI buffer
sweep (tests/abi_cases.py): differentiable reference scores, the kink-aware fp64 gradients (a pre-activation within KINK_TAU
of zero may take either ReLU sub-gradient; the best assignment is found by least squares) and GRAD_RTOL."""
import torch

GRAD_RTOL = 2e-4


def ref_scores(vs, ft, R, W1, W2, b2):
    """Differentiable reference: per sample rotate -> forward_3d2d -> mean cosine with ft (B,32,64)."""
    from oracle import torch_ref
    B = vs.shape[0]
    out = []
    for b in range(B):
        Rb = R[b] if R.dim() == 4 else R
        n = Rb.shape[0]
        rot = torch_ref.rotate_volume(vs[b][None].expand(n, -1, -1, -1, -1), Rb)
        f = torch_ref.forward_3d2d(rot, W1, W2, b2)
        out.append((f * ft[b][None]).sum(dim=1).mean(dim=-1))
    return torch.stack(out)


KINK_TAU = 2e-6   # |pre-activation| below this (fp64 reference; typical magnitude ~1) = ambiguous sub-gradient
KINK_MAX = 64     # reference backward passes spent on one case


def ref_scores_masked(vs, ft, R, W1, W2, b2, flips=None):
    """ref_scores with the ReLU written as u * mask, mask = (u > 0) XOR flips; returns (scores, list of u)."""
    from oracle import torch_ref
    import torch.nn.functional as F
    out, us = [], []
    for b in range(vs.shape[0]):
        Rb = R[b] if R.dim() == 4 else R
        n = Rb.shape[0]
        vol = torch_ref.rotate_volume(vs[b][None].expand(n, -1, -1, -1, -1), Rb)
        m, c, d, h, w = vol.shape
        slabs = torch.cat([vol.permute(0, 1, 4, 2, 3).reshape(m, c * w, d, h), vol.permute(0, 1, 3, 2, 4).reshape(m, c * h, d, w),
                           vol.reshape(m, c * d, h, w)], dim=1)                       # modules/modules.py:115-118
        u = F.conv2d(slabs, W1.reshape(32, 384, 1, 1))
        mask = (u.detach() > 0)
        if flips is not None:
            mask = mask ^ flips[b]
        v = F.conv2d(u * mask, W2.reshape(32, 32, 1, 1), b2)
        f = F.normalize(v, p=2, dim=1).flatten(2)
        out.append((f * ft[b][None]).sum(dim=1).mean(dim=-1))
        us.append(u.detach())
    return torch.stack(out), us


class KinkReference:
    """The fp64 gradients of one case, the list of its ambiguous ReLU sub-gradients and (lazily, once) the change of the
    gradients when each of them flips: several kernel results of the same case share one reference.
    A pre-activation of EXACTLY 0 is not ambiguous (tests/test_gpu_rotation_grad.py says the same): a rank-deficient R
    produces them, F.relu's sub-gradient there is 0 and so is the kernel's ``u > 0`` mask -- the fp64 reference and the
    kernel cannot take different sides."""

    def __init__(self, vs, ft, R, W1, W2, b2, gs, scale=1.0):
        self.args = (vs, ft, R, W1, W2, b2, gs)
        self.base, self.us = self.grads(None)
        self.rescale(scale)

    def rescale(self, scale):
        """KINK_TAU is stated for pre-activations of magnitude about 1; a case whose pre-activations are `scale` times that
        (tests/backward_cases.py: the clamp cases have u ~ 3e-13) lists those below KINK_TAU * scale."""
        self.scale = scale
        self.amb = [(b, idx) for b, u in enumerate(self.us) for idx in torch.nonzero((u.abs() < KINK_TAU * scale) & (u != 0)).tolist()]
        self.deltas = None

    def grads(self, flips):
        vs, ft, R, W1, W2, b2, gs = self.args
        leaves = [x.double().requires_grad_(True) for x in (vs, ft, W1, W2, b2)]
        s, us = ref_scores_masked(leaves[0], leaves[1], R.double(), leaves[2], leaves[3], leaves[4], flips)
        return torch.autograd.grad(s, leaves, grad_outputs=gs.double()), us

    def delta(self, b, idx):
        """The change of the five gradients when the sub-gradient of pre-activation `idx` of sample b flips."""
        flips = [torch.zeros_like(u, dtype=torch.bool) for u in self.us]
        flips[b][tuple(idx)] = True
        g, _ = self.grads(flips)
        return [x - y for x, y in zip(g, self.base)]

    def fit(self, got, bars=None):
        """(the reference under the best assignment of the ambiguous sub-gradients, how many there are, how many were
        flipped).  The plain fp64 gradients where nothing is ambiguous or `got` already agrees: within GRAD_RTOL, or within
        `bars` (one per gradient) where a caller holds the result to tighter ones."""
        base, us, amb = self.base, self.us, self.amb
        errs0 = [relerr(a, r.reshape(a.shape)) for a, r in zip(got, base)]
        agrees = max(errs0) < GRAD_RTOL if bars is None else all(e <= b for e, b in zip(errs0, bars))
        if not amb or agrees:
            return base, len(amb), 0
        assert len(amb) <= KINK_MAX, "too many near-kink pre-activations: %d" % len(amb)
        if self.deltas is None:
            self.deltas = [self.delta(b, idx) for b, idx in amb]
        deltas = self.deltas
        # the gradient is affine in the flip bits: least squares for the bits, rounded to {0, 1}
        flat = lambda ts: torch.cat([t.reshape(-1).double() for t in ts])
        A = torch.stack([flat(d) for d in deltas], dim=1)
        rhs = flat([a.double() - r.reshape(a.shape) for a, r in zip(got, base)])
        bits = (torch.linalg.lstsq(A, rhs[:, None]).solution[:, 0] > 0.5)
        ref = [x.clone() for x in base]
        for i in torch.nonzero(bits).flatten().tolist():
            ref = [x + d for x, d in zip(ref, deltas[i])]
        return ref, len(amb), int(bits.sum())

    def errors(self, got, bars=None):
        ref, n_amb, flipped = self.fit(got, bars)
        return [relerr(a, r.reshape(a.shape)) for a, r in zip(got, ref)], n_amb, flipped


def kink_aware_errors(got, vs, ft, R, W1, W2, b2, gs):
    """max relative error of every gradient against the best assignment of the ambiguous ReLU sub-gradients."""
    return KinkReference(vs, ft, R, W1, W2, b2, gs).errors(got)


def relerr(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
