"""tests/ff_train_cases.py checked on the CPU: the references agree with each other inside a written-down range, every
data kind is what its name says, the sizes cover what they claim, and the cases are the stock module's arithmetic."""
import pytest
import torch

from . import ff_train_cases as fc
from .backward_cases import PARITY_FACTOR
from .backward_reference import GRAD_RTOL


@pytest.mark.parametrize("kind,B", fc.all_cases())
def test_e_ref_inside_the_measured_range(kind, B):
    """ref32 against ref64: every e_ref within a factor of two of what was measured, and the bar follows from it."""
    c = fc.case(kind, B)
    for k in fc.TENSORS:
        lo, hi = fc.E_REF_MEASURED[k]
        print("%s B=%d %-3s e_ref %.3e  range [%.1e, %.1e]" % (kind, B, k, c.e_ref[k], lo / 2, 2 * hi))
        assert lo / 2 <= c.e_ref[k] <= 2 * hi, (kind, B, k, c.e_ref[k])
        assert c.bars[k] == min(GRAD_RTOL, PARITY_FACTOR * c.e_ref[k]) < GRAD_RTOL
        assert c.ref64[k].dtype == torch.float64 and c.ref32[k].dtype == torch.float32
        assert c.ref64[k].shape == c.ref32[k].shape and bool(torch.isfinite(c.ref64[k]).all())


def test_sizes_and_shapes():
    assert fc.SIZES == tuple(sorted(set(fc.SIZES))) and {1, 3, 9, 16, 17, 33} <= set(fc.SIZES)
    assert fc.TOKENS * 1 < 128 < fc.TOKENS * 3 and (fc.TOKENS * 3) % 128 != 0     # under one 128-row tile; one and a half
    assert fc.TOKENS * 16 == 1024 and fc.TOKENS * 17 > 1024 and fc.TOKENS * 33 == 2112
    cases = fc.all_cases()
    assert len(cases) == len(set(cases)) == len(fc.SIZES) + len(fc.KINDS) - 1
    c = fc.case("plain", 3)
    assert c.M == 192 and c.x.shape == (3, 64, 512) and c.gy.shape == (3, 64, 256)
    assert c.w1.shape == (4096, 512) and c.b1.shape == (4096,) and c.w2.shape == (256, 2048) and c.b2.shape == (256,)
    shapes = {"y": (192, 256), "dx": (192, 512), "dw1": (4096, 512), "db1": (4096,), "dw2": (256, 2048), "db2": (256,)}
    assert {k: tuple(v.shape) for k, v in c.ref64.items()} == shapes
    assert fc.case("plain", 3) is c                                     # built once, shared
    assert not torch.equal(c.x, fc.case("zero_bias", 3).x)              # seeded per (kind, B)
    again = fc.Case("plain", 3)
    assert torch.equal(again.x, c.x) and torch.equal(again.w1, c.w1) and torch.equal(again.ref32["dw2"], c.ref32["dw2"])


def test_wide_gate_reaches_both_tails():
    """|gate| > 8 on both sides (gelu' underflows, gelu saturates), and the dip of gelu near -0.75 is populated."""
    plain, wide = fc.case("plain", 3), fc.case("wide_gate", 3)
    g = wide.gates()
    assert g.min().item() < -8.0 and g.max().item() > 8.0
    assert int((g < -8.0).sum()) > 1000 and int((g > 8.0).sum()) > 1000
    assert int(((g > -1.0) & (g < -0.5)).sum()) > 1000
    assert plain.gates().abs().max().item() < 8.0 / 2
    lim =1.0 / fc.FF_IN ** 0.5                                          # nn.Linear's default: U(-1/sqrt(in), 1/sqrt(in))
    assert wide.w1[:fc.FF_INNER].abs().max().item() <= lim
    assert lim < wide.w1[fc.FF_INNER:].abs().max().item() <= fc.WIDE_GATE_SCALE * lim
    # the tails are what make the case: gelu'(g) is exactly 0 / 1 in fp32 out there, and the reference still has signal
    assert wide.ref64["dw1"][fc.FF_INNER:].abs().max().item() > 0


def test_zero_bias_and_sparse_grad_are_what_they_say():
    z = fc.case("zero_bias", 3)
    assert not z.b1.any() and not z.b2.any() and z.ref64["db1"].abs().max().item() > 0
    s = fc.case("sparse_grad", 3)
    assert not s.gy[:, 1::2].any() and bool(s.gy[:, 0::2].any())
    dx = s.ref64["dx"].reshape(3, 64, 512)
    assert not dx[:, 1::2].any() and bool(dx[:, 0::2].any())            # no gradient reaches a token without one
    assert fc.case("plain", 3).b1.any() and fc.case("plain", 3).gy[:, 1::2].any()


def test_references_are_the_stock_module_and_the_written_rule():
    """ref64 equals the arithmetic spelled out (exact erf GELU, gelu'(g) = Phi(g) + g phi(g)) to fp64 rounding."""
    c = fc.case("wide_gate", 3)
    x, gy = c.x.double().reshape(c.M, -1), c.gy.double().reshape(c.M, -1)
    w1, b1, w2, b2 = c.w1.double(), c.b1.double(), c.w2.double(), c.b2.double()
    pre = x @ w1.t() + b1
    val, gate = pre[:, :fc.FF_INNER], pre[:, fc.FF_INNER:]
    Phi = 0.5 * torch.special.erfc(-gate / 2 ** 0.5)
    phi = torch.exp(-0.5 * gate * gate) / (2 * torch.pi) ** 0.5
    act = val * gate * Phi
    dA = gy @ w2
    dP = torch.cat([dA * gate * Phi, dA * val * (Phi + gate * phi)], dim=1)
    want = {"y": act @ w2.t() + b2, "dx": dP @ w1, "dw1": dP.t() @ x, "db1": dP.sum(0), "dw2": gy.t() @ act, "db2": gy.sum(0)}
    errs = c.errors(want)
    assert max(errs.values()) < 1e-13, errs
    assert set(errs) == set(fc.TENSORS)
