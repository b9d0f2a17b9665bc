"""The pin that the gradient of the restatement is the reference's: tests/golden/rotation_grad.npz holds d score / d R
produced by the reference's OWN utils.rotate_volume (utils.py:113-131) and Feature_Aligner.forward_3d2d
(modules/modules.py:112-124) under torch autograd (tools/gen_golden.py gen_rotation_grad; inputs of score_n128, its first 32
rotations and the edge_rotations set), once as shipped in fp32 and once with the modules cast to fp64.  Every gradient
reference of the GPU tests goes through oracle/torch_ref.py and the slab lines restated in
tests/test_gpu_rotation_grad.py::ref_rotation_grad; here that restatement must reproduce the file.  No GPU needed.

Bars: fp64 against fp64 is the same ATen operators in the same order, so only the last bits may differ: 1e-10 of a
hypothesis' largest entry (fp64 epsilon 2e-16 times sums of a few thousand terms, with a wide margin).  The fp32 file against the fp64
restatement is stock torch fp32 against fp64, the yardstick of test_gpu_rotation_grad: its PARITY_BAR."""
import numpy as np
import torch

from .conftest import load_golden
from .test_gpu_rotation_grad import PARITY_BAR, check_ambiguous, hyp_err, ref_rotation_grad


def _inputs():
    g, r = load_golden("score_n128"), load_golden("rotation_grad")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return g, r, t


def test_golden_is_what_it_says():
    g, r, _ = _inputs()
    e = load_golden("edge_rotations")
    assert r["R"].shape == (65, 3, 3) and r["grad_R"].dtype == np.float32 and r["grad_R_f64"].dtype == np.float64
    assert np.array_equal(r["R"][:32], g["R"][:32]) and np.array_equal(r["R"][32:], e["R"])
    assert [str(n) for n in r["names"][32:]] == [str(n) for n in e["names"]]
    # the scores recorded beside the gradients are the reference's scores of the same hypotheses
    assert np.allclose(r["scores"][:32], g["scores"][0, :32], rtol=0, atol=1e-6)
    assert np.allclose(r["scores"][32:], e["scores"][0], rtol=0, atol=1e-6)
    assert np.isfinite(r["grad_R"]).all() and np.isfinite(r["grad_R_f64"]).all()


def test_restatement_gradient_is_the_references():
    from oracle import torch_ref
    g, r, t = _inputs()
    vs, W1, W2, b2, R = t(g["vol_src"]), t(g["W1"]), t(g["W2"]), t(g["b2"]), t(r["R"])
    with torch.no_grad():   # the fp64 run of the generator built its target features in fp64 too
        ft64 = torch_ref.forward_3d2d(t(g["vol_tgt"]).double(), W1.double(), W2.double(), b2.double())
    ref, amb = ref_rotation_grad(vs, ft64, R, W1, W2, b2)
    check_ambiguous("golden", amb, [str(n) for n in r["names"]])
    e64 = hyp_err(torch.from_numpy(r["grad_R_f64"])[None], ref)
    assert e64.max().item() <= 1e-10, e64.max().item()       # every hypothesis, the ambiguous ones included
    e32 = hyp_err(torch.from_numpy(r["grad_R"])[None], ref)
    assert e32[~amb].max().item() <= PARITY_BAR, e32[~amb].max().item()
    # and through the fp32 target features the reference stored (what the GPU test feeds the kernel): same gradient to 1e-6
    ref32ft, _ = ref_rotation_grad(vs, t(g["f_tgt"]), R, W1, W2, b2)
    assert hyp_err(ref32ft, ref).max().item() <= 1e-6
