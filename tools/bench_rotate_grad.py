"""What the rotation gradient of the op-level rotate_volume costs (profiles/rotate_grad.jsonl).  The method is
tools/bench_topk.py's: one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the rounds, min / max the
spread), time-based warm-up, device events around ``iters`` calls.

Three sets on (16, 8, 8, 8) volumes: one shared volume at N = 9 000 and N = 50 000, per-sample volumes at N = 9 000.  Per set:
  kernel            ops.rotate_volume_rotation_grad alone (ahv_rotate_volume_rotation_grad_f32) on resident grad_out
  autograd          ops.rotate_volume_autograd(vol, R).backward(g), only R requiring grad: forward + the kernel
  autograd_bwd      the backward of that graph alone (torch.autograd.grad on a retained graph)
  stock             what a user can do without it on the same GPU: F.affine_grid + F.grid_sample (PyTorch-ROCm) forward and
                    .backward(g), only R requiring grad
  stock_bwd         the backward of that graph alone
  volume_adjoint    ahv_rotate_volume_backward_f32 on the same set (the gradient that existed already), for scale
"gbytes_per_s" of the kernel rows: the 32 KiB of grad_out per hypothesis the kernel must read, over the kernel's time
(a per-sample set reads another 32 KiB of volume per hypothesis: "gbytes_per_s_with_volume").
The bar: kernel_path (autograd) faster than stock at both N by more than the spread between rounds.

``--lib`` measures another build of the same ABI, ``--variants`` a comma-separated subset (the rows that need "stock" are
then left without their ratios), ``--label`` is written into every row.

    python tools/bench_rotate_grad.py [--out profiles/rotate_grad.jsonl] [--rounds 5] [--iters 10] [--lib PATH] [--variants kernel,volume_adjoint] [--label NAME]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_topk import alternate  # noqa: E402  (same warm-up, same windows)

VOL = (16, 8, 8, 8)
VOL_BYTES = 4 * 16 * 512
SETS = [("shared", 9_000), ("shared", 50_000), ("per_sample", 9_000)]


def stock_rotate(volume, R):
    """utils.py:113-131 in stock operators (the reference's own lines)."""
    theta = torch.cat([R, R.new_zeros(R.shape[0], 3, 1)], dim=-1)
    grid = F.affine_grid(theta, list(volume.shape), align_corners=False)
    return F.grid_sample(volume, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rotate_grad.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lib", default=None, help="libahv_hip.so to measure instead of the in-tree build")
    ap.add_argument("--variants", default="", help="comma-separated subset of the variants")
    ap.add_argument("--label", default=None, help="build label written into every row")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rotate_grad.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    if a.lib:
        ahv._lib.LIB_PATH = os.path.abspath(a.lib)
    ops = ahv.ops
    dev = torch.device("cuda:0")
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count()}
    if a.label:
        box["build"] = a.label
    rows = []
    for kind, N in SETS:
        gen = torch.Generator(device=dev).manual_seed(N + len(kind))
        R = torch.from_numpy(ahv.rotations.haar_rotations_np(N, 7)).to(dev)
        if kind == "shared":
            vol = (torch.randn(VOL, device=dev, generator=gen) * 1.1)[None].expand(N, -1, -1, -1, -1)
        else:
            vol = torch.randn((N,) + VOL, device=dev, generator=gen) * 1.1
        g = torch.randn((N,) + VOL, device=dev, generator=gen)
        stride = 0 if kind == "shared" else 16 * 512
        gv = torch.empty((1 if kind == "shared" else N,) + VOL, dtype=torch.float32, device=dev)
        Rl = R.clone().requires_grad_(True)
        ours, stock = ops.rotate_volume_autograd(vol, Rl), stock_rotate(vol, Rl)
        # the two paths compute the same thing (to the tests' bar; measured here on the timed set itself)
        want = torch.autograd.grad(stock, Rl, g, retain_graph=True)[0]
        got = ops.rotate_volume_rotation_grad(vol, R, g)
        err = ((got - want).abs().flatten(1).max(dim=1).values / want.abs().flatten(1).max(dim=1).values.clamp_min(1e-30))

        def whole(fn):
            def f():
                r = R.detach().requires_grad_(True)
                fn(vol, r).backward(g)
                return r.grad
            return f

        variants = {
            "kernel": lambda: ops.rotate_volume_rotation_grad(vol, R, g),
            "autograd": whole(ops.rotate_volume_autograd),
            "autograd_bwd": lambda: torch.autograd.grad(ours, Rl, g, retain_graph=True),
            "stock": whole(stock_rotate),
            "stock_bwd": lambda: torch.autograd.grad(stock, Rl, g, retain_graph=True),
            "volume_adjoint": lambda: ops._call(dev, "ahv_rotate_volume_backward_f32", g.data_ptr(), stride, R.data_ptr(), N,
                                                16, 8, 8, 8, gv.data_ptr()),
        }
        if a.variants:
            variants = {k: variants[k] for k in a.variants.split(",")}
        st = alternate(variants, a.rounds, a.iters)
        for name, s in st.items():
            row = dict({"set": kind, "N": N, "variant": name}, **s, **box)
            if name in ("kernel", "volume_adjoint"):
                row["gbytes_per_s"] = round(N * VOL_BYTES / (s["us"] * 1e-6) / 1e9, 1)
                if kind != "shared" and name == "kernel":
                    row["gbytes_per_s_with_volume"] = round(2 * N * VOL_BYTES / (s["us"] * 1e-6) / 1e9, 1)
            if name == "autograd" and "stock" in st:
                row["stock_over_kernel_path"] = round(st["stock"]["us"] / s["us"], 2)
                row["faster_beyond_spread"] = bool(s["max_us"] < st["stock"]["min_us"])
                row["median_rel_err_vs_stock"] = float(err.median())
            rows.append(row)
            print(json.dumps(row), flush=True)
        del ours, stock, want, got, g, vol, gv
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
