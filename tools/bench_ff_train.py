"""What stock torch spends on the encoder's feed-forward under autograd (profiles/ff_train.jsonl): the baseline a HIP
forward + backward of ``aligner._FF`` has to beat.  The method is tools/bench_topk.py's: one process, one GPU, profiler off,
the variants timed ALTERNATELY over several rounds (the median of the rounds is the figure, min / max the spread),
time-based warm-up.

  F   one ``_FF(512, 256)`` (Linear 512 -> 2 x 2048, val * gelu(gate), Linear 2048 -> 256) at M = 64 B token rows, B = 12 and
      32: forward with autograd recording, and forward + backward into the gradients of the input and the four parameters;
      with hipBLASLt (torch's default) and with rocBLAS (what harness.fit selects).  "tflops" is the algorithmic rate
      (2 x 2.62 M MAC per token forward, three times that forward + backward), "frac_fp32_matrix_peak" its share of 157.3 TF.
  E   the encoder's token stage and projections (``BidirectionTransformer(256, 4, 64, depth=4)``, 16 feed-forwards) forward +
      backward at the same B, and ``ff_share`` = 16 x the F figure of the same BLAS over it.

    python tools/bench_ff_train.py [--out profiles/ff_train.jsonl] [--only F,E] [--rounds 5] [--iters 50]
"""
import argparse
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_topk import alternate  # noqa: E402  (same warm-up, same windows)

PEAK_TF = 157.3                       # fp32 matrix peak of the MI355X
MAC_PER_TOKEN = 512 * 4096 + 2048 * 256
BLAS = {"cublaslt": "hipBLASLt", "cublas": "rocBLAS"}
N_FF = 16                             # feed-forwards of a depth-4 encoder: four blocks per bidirectional block


def ff_flop(M, what):
    """Algorithmic FLOP of one ``_FF`` over M token rows: two per MAC forward, the backward's five products twice that."""
    return 2.0 * M * MAC_PER_TOKEN * {"fwd": 1, "fwd_bwd": 3}[what]


def ff_row(B, what, blas, stats):
    """Row F from the window statistics of ``alternate`` (``stats["us"]`` is the median)."""
    tf = ff_flop(64 * B, what) / stats["us"] / 1e6
    return dict({"row": "F", "what": "stock _FF " + what, "B": B, "M": 64 * B, "blas": BLAS[blas], "tflops": round(tf, 2),
                 "frac_fp32_matrix_peak": round(tf / PEAK_TF, 4)}, **stats)


def encoder_row(B, blas, stats, ff_fwd_bwd_us=None):
    """Row E; ``ff_share`` = 16 feed-forwards at the F figure of the same B and BLAS over the stage's time."""
    row = {"row": "E", "what": "stock encoder token stage fwd_bwd (depth 4, 16 feed-forwards)", "B": B, "blas": BLAS[blas]}
    if ff_fwd_bwd_us is not None:
        row["ff_share"] = round(N_FF * ff_fwd_bwd_us / stats["us"], 3)
    return dict(row, **stats)


def measure(only="", rounds=5, iters=50, batches=(12, 32), emit=None):
    """The rows of one run, in the order they were measured; ``emit(row)`` is called as each one is ready."""
    aligner = importlib.import_module("3dahv_amd.aligner")
    dev = torch.device("cuda:0")
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__}
    want = lambda r: not only or r in only.split(",")
    rows, ff_us = [], {}
    prev_blas = torch.backends.cuda.preferred_blas_library()

    def add(row):
        rows.append(dict(row, **box))
        if emit is not None:
            emit(rows[-1])

    def with_blas(blas, fn):
        def run():
            torch.backends.cuda.preferred_blas_library(blas)
            fn()
        return run

    try:
        for B in batches:
            torch.manual_seed(B)
            if want("F"):
                ff = aligner._FF(512, 256).to(dev).train()
                x = torch.randn(B, 64, 512, device=dev, requires_grad=True)
                gy = torch.randn(B, 64, 256, device=dev)
                leaves = [x] + list(ff.parameters())

                def fwd():
                    return ff(x)

                def fwd_bwd():
                    for t in leaves:
                        t.grad = None
                    ff(x).backward(gy)

                variants = {}
                for blas in BLAS:
                    variants["fwd/" + blas] = with_blas(blas, fwd)
                    variants["fwd_bwd/" + blas] = with_blas(blas, fwd_bwd)
                for name, st in alternate(variants, rounds, iters).items():
                    what, blas = name.split("/")
                    if what == "fwd_bwd":
                        ff_us[(B, blas)] = st["us"]
                    add(ff_row(B, what, blas, st))
            if want("E"):
                enc = aligner.BidirectionTransformer(256, 4, 64, depth=4).to(dev).train()
                xs = torch.randn(B, 256, 8, 8, device=dev, requires_grad=True)
                cs = torch.randn(B, 256, 8, 8, device=dev, requires_grad=True)
                gx, gc = torch.randn_like(xs), torch.randn_like(cs)
                eleaves = [xs, cs] + list(enc.parameters())

                def enc_fwd_bwd():
                    for t in eleaves:
                        t.grad = None
                    ox, oc = enc(xs, cs)
                    torch.autograd.backward([ox, oc], [gx, gc])

                variants = {"enc_fwd_bwd/" + blas: with_blas(blas, enc_fwd_bwd) for blas in BLAS}
                for name, st in alternate(variants, rounds, max(iters // 5, 1)).items():
                    blas = name.split("/")[1]
                    add(encoder_row(B, blas, st, ff_us.get((B, blas))))
    finally:
        torch.backends.cuda.preferred_blas_library(prev_blas)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ff_train.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ff_train.py measures on the GPU only")
    rows = measure(a.only, a.rounds, a.iters, emit=lambda r: print(json.dumps(r), flush=True))
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
