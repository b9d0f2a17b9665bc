"""The GELU of the encoder's GEGLU epilogues (csrc/ahv_enc_linear.h::gelu_pk) pinned on the CPU: the coefficients are
read out of the kernel source, the same Horner chain is evaluated with fp32 rounding after every fused multiply-add
(as tools/fit_gelu.py::gelu_pk does -- that module imports scipy at its top, so the chain is repeated here) and the result
is held to torch's GELU in fp64.  A mistyped coefficient moves GELU by ~1e-4, which no network-level bound can see.

With the committed coefficients: max |gelu_pk - fp64| = 2.55e-7 on [-300, 300] against 4.5e-7 for the fp32 expression
0.5 g (1 + erf(g / sqrt 2)).
"""
import os
import re

import numpy as np
import torch

from .conftest import REPO

SOURCE = os.path.join(REPO, "3dahv_amd", "csrc", "ahv_enc_linear.h")
f32 = np.float32
_NUM = r"([-+]?[0-9]+\.[0-9]+(?:e[-+]?[0-9]+)?)f"


def read_coefficients():
    """([c1 .. c8], constant) of gelu_pk's chain  r = c8 t + c7;  r = r t + c6; ...; r = r t + c1;  r = r t + constant.
    Every statement of the function is matched: a change of its shape fails here, not in the numbers below."""
    text = open(SOURCE).read()
    m = re.search(r"__device__ __forceinline__ f32x2 gelu_pk\(f32x2 g\)\n\{\n(.*?)\n\}\n", text, re.S)
    assert m, "gelu_pk(f32x2 g) not found in ahv_enc_linear.h: this test reads its coefficients from the source"
    lines = [ln.strip() for ln in m.group(1).split("\n") if ln.strip()]
    assert len(lines) == 12, "gelu_pk has changed shape (%d statements, 12 expected):\n%s" % (len(lines), m.group(1))
    assert lines[0] == "const f32x2 t = __builtin_elementwise_abs(g);", lines[0]
    first = re.fullmatch(r"f32x2 r = pk_fma\(AHV_PK\(%s\), t, AHV_PK\(%s\)\);" % (_NUM, _NUM), lines[1])
    assert first, "first step of the Horner chain: " + lines[1]
    chain = [float(first.group(1)), float(first.group(2))]
    for ln in lines[2:9]:
        step = re.fullmatch(r"r = pk_fma\(r, t, AHV_PK\(%s\)\);" % _NUM, ln)
        assert step, "Horner step: " + ln
        chain.append(float(step.group(1)))
    assert re.fullmatch(r"const f32x2 tail = \{__builtin_amdgcn_exp2f\(r\[0\]\), __builtin_amdgcn_exp2f\(r\[1\]\)\};.*", lines[9]), lines[9]
    assert lines[10] == "const f32x2 pos = {fmaxf(g[0], 0.0f), fmaxf(g[1], 0.0f)};", lines[10]
    assert lines[11] == "return pk_fma(-t, tail, pos);", lines[11]
    assert len(chain) == 9
    return [f32(c) for c in chain[7::-1]], f32(chain[8])   # c1 .. c8, constant


def fma(a, b, c):
    """One fused multiply-add with an fp32 result (the product of two fp32 values is exact in fp64)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def poly32(t, cs, const):
    r = np.full_like(t, cs[-1])
    for k in range(len(cs) - 2, -1, -1):
        r = fma(r, t, cs[k])
    return fma(r, t, const)


def gelu_pk(g, cs, const):
    g = g.astype(f32)
    t = np.abs(g)
    r = poly32(t, cs, const)
    with np.errstate(all="ignore"):
        e = np.exp2(r.astype(np.float64)).astype(f32)
    return fma(-t, e, np.maximum(g, f32(0)))


def gelu64(g):
    return torch.nn.functional.gelu(torch.from_numpy(g.astype(np.float64))).numpy()


def gelu_expression_fp32(g):
    """0.5 g (1 + erf(g / sqrt 2)) with every operation in fp32: the expression F.gelu evaluates for an fp32 tensor."""
    t = torch.from_numpy(g.astype(f32))
    return (0.5 * t * (1.0 + torch.erf(t * f32(0.70710678118654752)))).numpy()


def test_constant_and_signs_read_from_the_source():
    cs, const = read_coefficients()
    assert const == f32(-1.0)       # Phi(0) = 1/2 = exp2(-1)
    assert len(cs) == 8 and cs[7] < 0   # c8 < 0: the polynomial falls beyond the fitted range, exp2 -> 0 without a clamp
    # p'(0) = d/dt log2 Phi(-t) at 0 = -(phi(0) / Phi(0)) / ln 2 = -sqrt(2 / pi) * 2 / (2 ln 2)
    assert abs(float(cs[0]) + np.sqrt(2.0 / np.pi) / np.log(2.0)) < 1e-3


def test_gelu_pk_against_fp64_gelu():
    cs, const = read_coefficients()
    dense = np.linspace(-12, 12, 2_000_001).astype(f32)
    wide = np.linspace(-300, 300, 200_001).astype(f32)
    edge = np.array([1e4, 1e10, 3e38, 0.0, 1e-40], dtype=f32)   # 1e-40: subnormal in fp32
    edge = np.concatenate([edge, -edge])
    for g in (dense, wide, edge):
        assert np.isfinite(gelu_pk(g, cs, const)).all()
    y_edge = gelu_pk(edge, cs, const)
    for v in (-1e4, -1e10, -3e38):
        assert y_edge[edge == f32(v)][0] == 0.0, v             # large negatives: exactly 0 (exp2 underflows, nothing cancels)
    for v in (1e4, 1e10, 3e38):
        assert y_edge[edge == f32(v)][0] == f32(v), v          # large positives: the value itself
    assert np.all(y_edge[np.abs(edge) <= f32(1e-40)] == 0.5 * edge[np.abs(edge) <= f32(1e-40)])   # GELU(g) -> g / 2 at 0
    assert np.all(gelu_pk(wide[wide < -40], cs, const) == 0.0)
    g = np.concatenate([dense, wide])
    ref = gelu64(g)
    e_pk = np.abs(gelu_pk(g, cs, const).astype(np.float64) - ref).max()
    e_32 = np.abs(gelu_expression_fp32(g).astype(np.float64) - ref).max()
    print("max |gelu_pk - fp64| %.3e   max |fp32 expression - fp64| %.3e" % (e_pk, e_32))
    assert e_pk <= e_32, (e_pk, e_32)


def test_polynomial_falls_monotonically_beyond_the_fitted_range():
    cs, const = read_coefficients()
    t = np.linspace(6, 400, 100_001)
    p = sum(float(cs[k]) * t ** (k + 1) for k in range(8)) + float(const)
    assert np.all(np.diff(p) < 0)
    p32 = poly32(t.astype(f32), cs, const)                     # the chain as the kernel rounds it
    assert np.isfinite(p32).all() and np.all(np.diff(p32) <= 0) and p32[0] < -29   # log2 Phi(-6) = -29.9
