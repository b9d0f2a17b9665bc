"""fp64 truth, stock fp32 operators and the per-sample acceptance rule for the encoder's HIP kernels
(csrc/ahv_encoder.hip and its ahv_enc_*.h), shared by tests/test_gpu_encoder_batch.py.

The modules of 3dahv_amd/aligner.py route anything but fp32 inference on the GPU to stock torch operators, so the same
module in fp64 is the truth and the same module with its HIP switches off is the yardstick: a HIP result may be as far
from the fp64 result as THREE times the worst sample of the stock fp32 operators on the same inputs (the project's own
factor, tests/test_gpu_encoder.py::test_attention_with_saturated_softmax), per sample and with no additive floor.  The
stock error is recomputed at every call: nothing is calibrated against the code under test.
"""
import contextlib
import copy

import torch

FACTOR = 3.0
SCALES = (0.03, 0.3, 1.0, 3.0, 30.0)


def _run(m, a, b):
    """forward_2d3d of a Feature_Aligner (inference form), or m(a, b) of a BidirectionTransformer / block."""
    with torch.no_grad():
        if hasattr(m, "forward_2d3d"):
            return m.forward_2d3d(a, b, random_mask=False, mask_ratio=0.0)
        return m(a, b)


@contextlib.contextmanager
def _hip_switches(m, value):
    owners = [o for o in (m, getattr(m, "att", None)) if o is not None]
    names = [(o, n) for o in owners for n in ("use_hip_encoder", "use_hip") if hasattr(o, n)]
    saved = [getattr(o, n) for o, n in names]
    try:
        for o, n in names:
            setattr(o, n, value)
        yield
    finally:
        for (o, n), v in zip(names, saved):
            setattr(o, n, v)


def double_copy(m):
    """The module in fp64 (the position code stays as the module computes it: shared data)."""
    return copy.deepcopy(m).double()


def truth(fa, a, b, fa64=None):
    """fp64 result of the same module (pass `fa64 = double_copy(fa)` to reuse one copy over many calls)."""
    m = double_copy(fa) if fa64 is None else fa64
    return _run(m, a.double(), b.double())


def stock32(fa, a, b):
    """The same module on stock fp32 torch operators (use_hip_encoder = att.use_hip = False)."""
    with _hip_switches(fa, False):
        return _run(fa, a, b)


def hip32(fa, a, b):
    """The same module with every HIP switch on; fails when the call would not reach the HIP kernels."""
    with _hip_switches(fa, True), torch.no_grad():
        if hasattr(fa, "_hip_2d3d_eligible"):
            assert fa._hip_2d3d_eligible(a), "forward_2d3d would run stock operators here"
        else:
            assert fa._hip_eligible(torch.empty(a.shape[0], 64, 256, device=a.device)), "the token stage would run stock operators"
        return _run(fa, a, b)


def sample_errors(x, t):
    """(emax, erms), each of length B:  emax[i] = max|x_i - t_i| / max|t_i|,  erms[i] = rms(x_i - t_i) / rms(t_i)."""
    t = t.double().flatten(1)
    d = x.to(t.device).double().flatten(1) - t
    emax = d.abs().amax(1) / t.abs().amax(1)
    erms = d.pow(2).mean(1).sqrt() / t.pow(2).mean(1).sqrt()
    return emax, erms


def accept(x, s, t, what=""):
    """The acceptance rule for a HIP output `x`, the stock fp32 output `s` and the truth `t`: for every sample
    emax_hip[i] <= 3 max_j emax_stock[j] and the same for erms.  Returns (max emax_hip / max emax_stock,
    max erms_hip / max erms_stock), printed as well so that a run with -s records them."""
    assert x.shape == s.shape == t.shape and x.dtype == torch.float32 and s.dtype == torch.float32 and t.dtype == torch.float64
    assert torch.isfinite(x).all(), what + ": non-finite HIP output"
    (hmax, hrms), (smax, srms) = sample_errors(x, t), sample_errors(s, t)
    bmax, brms = smax.max().item(), srms.max().item()
    rmax, rrms = hmax.max().item() / bmax, hrms.max().item() / brms
    print("%s: emax hip %.3e stock %.3e ratio %.3f | erms hip %.3e stock %.3e ratio %.3f"
          % (what, hmax.max().item(), bmax, rmax, hrms.max().item(), brms, rrms))
    bad_max = (hmax > FACTOR * bmax).nonzero().flatten().tolist()
    bad_rms = (hrms > FACTOR * brms).nonzero().flatten().tolist()
    assert not bad_max, "%s: emax of samples %s = %s above %g x stock %.3e" % (what, bad_max, hmax[bad_max].tolist(), FACTOR, bmax)
    assert not bad_rms, "%s: erms of samples %s = %s above %g x stock %.3e" % (what, bad_rms, hrms[bad_rms].tolist(), FACTOR, brms)
    return rmax, rrms


def scaled_samples(B, shape, seed, first=0):
    """B independent randn(*shape) samples; sample i (counted from `first`) is scaled by SCALES[i % 5], so that a read
    from the wrong sample is not a small error."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, *shape, generator=g)
    f = torch.tensor([SCALES[(first + i) % len(SCALES)] for i in range(B)])
    return x * f.reshape(B, *([1] * len(shape)))
