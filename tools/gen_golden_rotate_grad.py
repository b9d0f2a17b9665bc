#!/usr/bin/env python3
"""Generate tests/golden/rotate_volume_grad.npz by running the REFERENCE's own ``utils.rotate_volume`` (utils.py:113-131:
F.affine_grid + F.grid_sample) under torch autograd on the CPU: the gradient w.r.t. ``rotation_matrix`` of
<grad_out, rotate_volume(vol_src.expand(N, ...), R)>.

Runs only where the reference checkout is present (tools/gen_golden.py's import_reference and its stubs for the
reference's unused imports).  Inputs: G1 `score_n128`'s vol_src, its first 32 rotations and the G3 `edge_rotations` set
(the 65 hypotheses of G12).  grad_out is drawn from the recorded seed -- tests/rotate_grad_reference.py::seeded_grad_out
-- and NOT stored, so the file stays a few kilobytes.  Stored: R, names, seed, grad_R of the run as shipped (fp32) and
grad_R_f64 of the same call on fp64 inputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden")
SEED = 409


def main():
    from gen_golden import import_reference
    from tests.rotate_grad_reference import seeded_grad_out
    rotate_volume, _ = import_reference()
    g1 = np.load(os.path.join(OUT, "score_n128.npz"))
    g3 = np.load(os.path.join(OUT, "edge_rotations.npz"))
    R = np.concatenate([g1["R"][:32], g3["R"]]).astype(np.float32)
    names = np.array(["haar%02d" % i for i in range(32)] + [str(n) for n in g3["names"]])
    n = R.shape[0]
    vol = torch.from_numpy(np.ascontiguousarray(g1["vol_src"]))          # (1,16,8,8,8)
    gout = seeded_grad_out(SEED, n)
    out = {}
    for tag, dtype in (("", torch.float32), ("_f64", torch.float64)):
        Rl = torch.from_numpy(R).to(dtype).requires_grad_(True)
        warped = rotate_volume(vol.to(dtype).expand(n, -1, -1, -1, -1), Rl)
        (g,) = torch.autograd.grad(warped, Rl, grad_outputs=gout.to(dtype))
        out["grad_R" + tag] = g.numpy()
    err = np.abs(out["grad_R"] - out["grad_R_f64"]).reshape(n, 9).max(1) / np.abs(out["grad_R_f64"]).reshape(n, 9).max(1).clip(1e-30)
    print("rotate_volume_grad: %d hypotheses, |grad| max %.3e, fp32 run against fp64 run: max %.2e"
          % (n, np.abs(out["grad_R_f64"]).max(), err.max()))
    np.savez(os.path.join(OUT, "rotate_volume_grad.npz"), R=R, names=names, seed=np.int64(SEED), **out)


if __name__ == "__main__":
    main()
