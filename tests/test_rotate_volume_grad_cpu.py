"""What can be said about the rotation gradient of the op-level rotate_volume without a GPU.

Golden pin: tests/golden/rotate_volume_grad.npz holds d <grad_out, rotate_volume(vol, R)> / d R produced by the reference's
OWN utils.rotate_volume (utils.py:113-131) under torch autograd (tools/gen_golden_rotate_grad.py: score_n128's vol_src, its
first 32 rotations and the edge_rotations set; grad_out re-created from the recorded seed), once as shipped in fp32 and
once in fp64.  The reference of the GPU tests (tests/rotate_grad_reference.py, through oracle/torch_ref.py) must reproduce the
fp64 file to 1e-10 of each hypothesis' largest entry -- the same ATen operators in the same order, the bar of
tests/test_rotation_grad_golden_cpu.py -- and the fp32 file lies within the GPU test's PARITY_BAR of it.

Then the C ABI (declaration, ctypes signature, export, argument checks before any HIP call) and the routing of the drop-in,
with the ``ops`` functions replaced: no kernel runs."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from . import rotate_grad_reference as rg
from .conftest import REPO, load_golden
from .test_gpu_rotate_volume_grad import PARITY_BAR

SYMBOL = "ahv_rotate_volume_rotation_grad_f32"


def test_golden_is_what_it_says():
    g, e, r = load_golden("score_n128"), load_golden("edge_rotations"), load_golden("rotate_volume_grad")
    assert sorted(r.files) == ["R", "grad_R", "grad_R_f64", "names", "seed"]
    assert r["R"].shape == (65, 3, 3) and r["grad_R"].dtype == np.float32 and r["grad_R_f64"].dtype == np.float64
    assert r["grad_R"].shape == r["grad_R_f64"].shape == (65, 3, 3)
    assert np.array_equal(r["R"][:32], g["R"][:32]) and np.array_equal(r["R"][32:], e["R"])
    assert [str(n) for n in r["names"][32:]] == [str(n) for n in e["names"]]
    assert np.isfinite(r["grad_R"]).all() and np.isfinite(r["grad_R_f64"]).all()
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "rotate_volume_grad.npz")) < 32 * 1024


def test_reference_gradient_is_the_references():
    g, r = load_golden("score_n128"), load_golden("rotate_volume_grad")
    R = torch.from_numpy(np.ascontiguousarray(r["R"]))
    names = [str(n) for n in r["names"]]
    vol = torch.from_numpy(np.ascontiguousarray(g["vol_src"]))[0]
    gout = rg.seeded_grad_out(int(r["seed"]), R.shape[0])
    ref = rg.ref_rotate_grad(vol, R, gout)
    amb = rg.ambiguous(R, 8, 8, 8)
    rg.check_ambiguous("golden", amb, names)
    e64 = rg.hyp_err(torch.from_numpy(r["grad_R_f64"]), ref)
    assert e64.max().item() <= 1e-10, e64.max().item()        # every hypothesis, the ambiguous ones included
    e32 = rg.hyp_err(torch.from_numpy(r["grad_R"]), ref)
    assert e32[~amb].max().item() <= PARITY_BAR, e32[~amb].max().item()
    # zero: every sample sits at the centre, the gradient is not zero (the derivative of the trilinear sample there)
    assert np.abs(r["grad_R_f64"][names.index("zero")]).max() > 0


def test_ambiguous_rule():
    eye = torch.eye(3)[None]
    assert not rg.ambiguous(eye, 8, 8, 8).any()                       # exactly integer coordinates
    assert rg.ambiguous(eye * (1 + 1e-7), 8, 8, 8).all()              # 3.5 * 1e-7 off an integer
    assert not rg.ambiguous(eye * 1.01, 8, 8, 8).any()
    with pytest.raises(AssertionError):
        rg.check_ambiguous("x", torch.tensor([True] + [False] * 18))              # a case under 20 hypotheses
    with pytest.raises(AssertionError):
        rg.check_ambiguous("x", torch.tensor([True] + [False] * 30), ["zero"] + ["r"] * 30)
    assert rg.check_ambiguous("x", torch.tensor([True] + [False] * 30)) == 1


# ---- C ABI -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def test_symbol_is_declared_typed_and_exported(lib, ahv):
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ahv.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, text)
    res, args = ahv._lib.SIGNATURES[SYMBOL]
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert res is i and args == [vp, vp, i64, vp, i64, i, i, i, i, vp, vp]
    out = subprocess.check_output(["nm", "-D", "--defined-only", ahv._lib.LIB_PATH], text=True)
    assert re.search(r" T %s$" % SYMBOL, out, flags=re.M)
    assert getattr(lib, SYMBOL).argtypes == args
    assert lib.ahv_abi_version() == (2 << 16) | 3       # added under 2.3: callers probe for the symbol


def test_argument_validation_needs_no_gpu(lib):
    f = getattr(lib, SYMBOL)
    err = lib.ahv_last_error
    # (grad_out, vol, vol_batch_stride, R, N, C, D, H, W, grad_R, stream); the pointers are never dereferenced here
    assert f(1, 1, 0, 1, -1, 16, 8, 8, 8, 1, None) == -1 and b"rotate_volume_rotation_grad: bad shape" in err()
    for bad in ((0, 8, 8, 8), (16, 0, 8, 8), (16, 8, -2, 8), (16, 8, 8, 0)):
        assert f(1, 1, 0, 1, 4, *bad, 1, None) == -1 and b"bad shape" in err()
    assert f(1, 1, 8191, 1, 4, 16, 8, 8, 8, 1, None) == -1 and b"batch stride" in err()
    assert f(1, 1, -8192, 1, 4, 16, 8, 8, 8, 1, None) == -1 and b"batch stride" in err()
    assert f(1, 1, 59, 1, 4, 3, 4, 5, 1, 1, None) == -1 and b"batch stride" in err()
    for null in (0, 1, 3, 9):
        a = [1, 1, 0, 1, 4, 16, 8, 8, 8, 1, None]
        a[null] = None
        assert f(*a) == -1 and b"null pointer" in err()
    # N = 0: nothing to do, pointers may be null, no launch (a stride that is wrong is still refused)
    assert f(None, None, 0, None, 0, 16, 8, 8, 8, None, None) == 0
    assert f(None, None, 8192, None, 0, 16, 8, 8, 8, None, None) == 0
    assert f(None, None, 5, None, 0, 16, 8, 8, 8, None, None) == -1


# ---- routing ---------------------------------------------------------------------------------------------
@pytest.fixture
def routed(ahv, monkeypatch):
    """``ops.rotate_volume`` / ``ops.rotate_volume_autograd`` replaced by recorders; patch.calls is left with the keys it
    had (the counter of the autograd route appears with its first call, and other tests compare the whole dict)."""
    seen = []
    monkeypatch.setattr(ahv.ops, "rotate_volume", lambda v, R, padding_mode="zeros": seen.append("plain") or "plain")
    monkeypatch.setattr(ahv.ops, "rotate_volume_autograd", lambda v, R, padding_mode="zeros": seen.append("autograd") or "autograd")
    had = "rotate_volume_autograd" in ahv.patch.calls
    try:
        yield seen
    finally:
        if not had:
            ahv.patch.calls.pop("rotate_volume_autograd", None)


@pytest.mark.parametrize("shared", [True, False])
def test_drop_in_routes_a_rotation_that_requires_grad(ahv, routed, shared):
    calls = ahv.patch.calls
    N = 4
    vol = torch.zeros(1, 16, 8, 8, 8).expand(N, -1, -1, -1, -1) if shared else torch.zeros(N, 3, 2, 2, 2)
    R = torch.eye(3)[None].repeat(N, 1, 1)
    Rg = R.clone().requires_grad_(True)
    n0, k0 = calls.get("rotate_volume_autograd", 0), calls["rotate_volume_kernel"]
    # (the deferral needs the device: on the CPU every call reaches the routing below it)
    assert ahv.patch._hip_rotate_volume(vol, Rg) == "autograd"
    assert calls["rotate_volume_autograd"] == n0 + 1 and calls["rotate_volume_kernel"] == k0
    assert ahv.patch._hip_rotate_volume(vol, R) == "plain"
    with torch.no_grad():
        assert ahv.patch._hip_rotate_volume(vol, Rg) == "plain"
    assert ahv.patch._hip_rotate_volume(vol.clone().requires_grad_(True), R) == "plain"    # the volume's edge: rotate_volume's own
    assert calls["rotate_volume_autograd"] == n0 + 1 and calls["rotate_volume_kernel"] == k0 + 3
    assert routed == ["autograd", "plain", "plain", "plain"]


def test_deferred_backend_routes_the_same_way(ahv, routed):
    be = ahv.deferred._hip_backend()
    vol = torch.zeros(1, 16, 8, 8, 8).expand(3, -1, -1, -1, -1)
    R = torch.eye(3)[None].repeat(3, 1, 1)
    assert be.rotate_volume(vol, R.clone().requires_grad_(True)) == "autograd"
    assert be.rotate_volume(vol, R) == "plain"
    with torch.no_grad():
        assert be.rotate_volume(vol, R.clone().requires_grad_(True)) == "plain"
    assert routed == ["autograd", "plain", "plain"]
    # a rotation that requires grad is never deferred: the call reaches the routing
    assert ahv.deferred.defer_rotate_volume(vol, R.clone().requires_grad_(True), be=ahv.deferred.Backend(
        rotate_volume=None, forward_3d2d=None, score_hypotheses=None, device_type="cpu"), allow_grad=True) is None


def test_rotate_volume_still_refuses_and_names_both_ways_out(ahv):
    vol = torch.zeros(2, 16, 8, 8, 8)
    R = torch.eye(3)[None].repeat(2, 1, 1).requires_grad_(True)
    with pytest.raises(NotImplementedError) as ei:
        ahv.ops.rotate_volume(vol, R)
    assert "score_hypotheses" in str(ei.value) and "rotate_volume_autograd" in str(ei.value)
    assert "rotate_volume_autograd" in ahv.ops.rotate_volume.__doc__


def test_op_layer_refuses_what_it_cannot_do(ahv):
    vol = torch.zeros(2, 16, 8, 8, 8)
    R = torch.eye(3)[None].repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.rotate_volume_rotation_grad(vol, R, torch.zeros_like(vol))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.rotate_volume_autograd(vol, R.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="padding_mode"):
        ahv.ops.rotate_volume_autograd(vol, R, padding_mode="border")
    with pytest.raises(RuntimeError, match="grad_out"):
        ahv.ops.rotate_volume_rotation_grad(vol, R, torch.zeros(2, 16, 8, 8, 4))
