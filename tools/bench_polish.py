"""What the rotation gradient and gradient-based polishing cost, and what they buy (profiles/polish_step.jsonl).  One process,
one GPU, profiler off; the variants of a row are timed ALTERNATELY over several rounds (median = the figure, min / max the
spread), every shape warmed first -- the method of tools/bench_topk.py, whose helpers this reuses.

  G   score_rotation_grad at B x N = 1 x 64, 1 x 1 024, 32 x 64, 32 x 1 024 in us, beside score_hypotheses on the same set
      ("x_scorer" = the ratio)
  P   verify_pair_polished at one pair x 50 000 for K in {1, 8, 16} x iters in {4, 8}, beside the plain arg-max step
      (verify_pair + select_rotation) timed in the same rounds; "added_us" = P - plain.  The plain step is timed on THIS
      build, not on a checkout of the parent commit: the feature leaves the fused scorer and the select untouched
      (ahv_score.hip is byte for byte the parent's), so the two builds run the same code for it; A / A2 give its spread
  Q   planted optimum (vol_tgt := rotate_volume(vol_src, R_gt), so score(R_gt) = 1 is the global maximum), several R_gt:
      score and geodesic error of (a) the 50 000 arg-max, (b) CoarseToFine 10 000 + 1 000, (c) arg-max + polish (K = 8,
      iters = 8), (d) CoarseToFine 10 000 + 1 000 + polish_iters = 8, each with its time

    python tools/bench_polish.py [--out profiles/polish_step.jsonl] [--only G,P,Q] [--rounds 5] [--iters 30] [--lib PATH] [--label NAME]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_topk import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "polish_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--lib", default=None, help="libahv_hip.so to measure instead of the in-tree build")
    ap.add_argument("--label", default=None, help="build label written into every row")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_polish.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    if a.lib:
        ahv._lib.LIB_PATH = os.path.abspath(a.lib)
    ops, rot = ahv.ops, ahv.rotations
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count()}
    if a.label:
        box["build"] = a.label
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")

    if want("G"):
        rng = np.random.RandomState(3)
        for B, N in ((1, 64), (1, 1024), (32, 64), (32, 1024)):
            v = T((rng.standard_normal((B, 16, 8, 8, 8)) * 1.1).astype(np.float32))
            ft = ops.forward_3d2d(T((rng.standard_normal((B, 16, 8, 8, 8)) * 1.1).astype(np.float32)), W1, W2, b2)
            R = T(rot.haar_rotations_np(N, 11))
            out = torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev)
            ws = torch.empty((2048 * B * N,), dtype=torch.float32, device=dev)
            st = alternate({"G_score_rotation_grad": lambda: ops.score_rotation_grad(v, ft, R, W1, W2, b2, out=out, workspace=ws),
                            "G_score_hypotheses": lambda: ops.score_hypotheses(v, ft, R, W1, W2, b2)}, a.rounds, a.iters)
            ratio = round(st["G_score_rotation_grad"]["us"] / st["G_score_hypotheses"]["us"], 2)
            for s in st.values():
                s["x_scorer"] = ratio
            emit({"row": "G", "B": B, "N": N}, st)

    if want("P"):
        N = 50_000
        R = T(rot.haar_rotations_np(N, 7))
        key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

        def plain():
            ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=False, best_key=key, reset_best=False)
            return ops.select_rotation(key, R, reset_key=True)

        variants = {"P_plain_argmax_step": plain, "P_plain_again": plain}
        for K in (1, 8, 16):
            for it in (4, 8):
                variants["P_polished_K%d_iters%d" % (K, it)] = \
                    lambda K=K, it=it: ops.verify_pair_polished(vs, vt, R, W1, W2, b2, K=K, iters=it)
        st = alternate(variants, a.rounds, a.iters)
        base = st["P_plain_argmax_step"]["us"]
        s0 = plain()[0].item()
        for name, s in st.items():
            s["added_us"] = round(s["us"] - base, 3)
            s["score"] = round(variants[name]()[0].item(), 6)
            s["score_plain"] = round(s0, 6)
        emit({"row": "P", "B": 1, "N": N}, st)

    if want("Q"):
        Rgt = torch.from_numpy(rot.haar_rotations_np(6, 4242))
        U, _, Vh = torch.linalg.svd(Rgt.double())
        Rgt64 = U @ Vh
        R50 = T(rot.haar_rotations_np(50_000, 7))
        R10 = T(rot.haar_rotations_np(10_000, 40))
        c2f = ahv.refine.CoarseToFine(W1, W2, b2, R10, n_fine=1000, batch=1, use_graph=False)
        c2f_p = ahv.refine.CoarseToFine(W1, W2, b2, R10, n_fine=1000, batch=1, use_graph=False, polish_iters=8)
        geo = lambda Rp, j: rot.geodesic_deg(Rp.double().cpu(), Rgt64[j:j + 1]).item()
        for j in range(Rgt.shape[0]):
            with torch.no_grad():
                tgt = ops.rotate_volume(vs, Rgt64[j:j + 1].float().to(dev))
            key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

            def argmax50():
                ops.verify_pair(vs, tgt, R50, W1, W2, b2, want_scores=False, best_key=key, reset_best=False)
                s, _, Rp = ops.select_rotation(key, R50, reset_key=True)
                return s, Rp

            variants = {"Q_a_argmax_50000": argmax50,
                        "Q_b_coarse_to_fine_10000_1000": lambda: (lambda o: (o[0], o[2]))(c2f(vs, tgt)),
                        "Q_c_argmax_50000_polish_K8_iters8":
                            lambda: ops.verify_pair_polished(vs, tgt, R50, W1, W2, b2, K=8, iters=8)[:2],
                        "Q_d_coarse_to_fine_polish_iters8": lambda: (lambda o: (o[0], o[2]))(c2f_p(vs, tgt))}
            st = alternate(variants, a.rounds, a.iters)
            for name, s in st.items():
                sc, Rp = variants[name]()
                s["score"] = round(sc.item(), 6)
                s["geodesic_err_deg"] = round(geo(Rp, j), 4)
            emit({"row": "Q", "pair": j}, st)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
