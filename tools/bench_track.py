"""What a tracker step costs, and what it buys (profiles/track_step.jsonl).  The method is tools/bench_resample.py's: one process,
one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max the spread), time-based warm-up.

One pair (tests/golden/score_n128.npz), B = 1:
  A   the per-frame step without a tracker: verify_pair on 50 000 Haar hypotheses + select_rotation      (the parent's code)
  B   PoseTracker.step at M = 512, 2 048, 4 096 particles (sigma 3 deg, 32 fresh slots, T = 0.02), eager and captured
  C   the same step with its glue in stock torch around the same scorer launch: softmax / cumsum / searchsorted for the draws,
      torch.randn for the noise, axis_angle_to_matrix + matmul for the move (fp32; its draws and noise are NOT the kernels' bit
      for bit), the elite and the fresh slots by indexing
      "kernel_minus_stock_us" = B eager - C; the bar: negative by more than the windows' spread ("spread_us", the widest
      max - min of the two rows) at every M.  "bar_met" records it per M, and a missed bar ends the run with exit status 1
      after the rows are written.
  Q   the planted moving optimum of tests/track_reference.py on the device: per-frame errors of the tracker and of the blind
      4 096-hypothesis arg-max, three sequences.  Reported without a bar (tests/test_gpu_track.py holds the bar).
B against A is reported, not barred.  The rows A, B and C are timed alternately in one block: naming any of them in --only
runs the block.

    python tools/bench_track.py [--out profiles/track_step.jsonl] [--only A,B,Q] [--rounds 5] [--iters 200]
"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_topk import alternate  # noqa: E402  (same warm-up, same windows)

SIGMA, N_FRESH, TEMP = 3.0, 32, 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_track.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "sigma_deg": SIGMA, "n_fresh": N_FRESH, "temperature": TEMP}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    beta = ops.inverse_temperature(TEMP)
    R0 = T(rot.haar_rotations_np(4096, 1000))

    def tracker(M, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=SIGMA, n_fresh=N_FRESH, temperature=TEMP, batch=1, seed=0, **kw)
        t.init(vs, vt, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(vs, vt)
        return t

    def stock_step(M):
        """The step's glue in stock torch; the scorer launch and select_rotation are the tracker's."""
        state = {"R": R0[None].expand(1, -1, -1, -1).contiguous(), "s": ops.verify_pair(vs, vt, R0, W1, W2, b2)[0],
                 "best": torch.zeros(1, dtype=torch.int64, device=dev)}
        key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)
        ar = (torch.arange(M, device=dev, dtype=torch.float32))[None]
        sig = math.radians(SIGMA)

        def f():
            R, s = state["R"], state["s"]
            u = torch.rand(1, 1, device=dev)
            c = torch.cumsum(torch.softmax(s * beta, dim=1), dim=1)
            idx = torch.searchsorted(c, ((ar + u) / M).contiguous(), right=True).clamp_(max=s.shape[1] - 1)
            w = torch.randn(M, 3, device=dev) * sig
            new = torch.matmul(R[0][idx[0]], rot.axis_angle_to_matrix(w))[None]
            new[:, 0] = R[0][state["best"]]
            new[:, M - N_FRESH:] = rot.random_rotations(N_FRESH, device=dev)[None]
            new = new.contiguous()
            s2, _ = ops.verify_pair(vs, vt, new, W1, W2, b2, want_scores=True, best_key=key, reset_best=True)
            sc, i, Rm = ops.select_rotation(key, new)
            state["R"], state["s"], state["best"] = new, s2, i
            return sc, i, Rm
        return f

    missed = []
    if want("A") or want("B") or want("C"):
        RA = T(rot.haar_rotations_np(50_000, 7))
        keyA = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

        def step_a():
            ops.verify_pair(vs, vt, RA, W1, W2, b2, want_scores=False, best_key=keyA, reset_best=False)
            return ops.select_rotation(keyA, RA, reset_key=True)

        for M in (512, 2048, 4096):
            te, tg = tracker(M), tracker(M, use_graph=True)
            variants = {"A_blind_50000": step_a, "B_tracker_eager": lambda t=te: t.step(vs, vt),
                        "B_tracker_captured": lambda t=tg: t.step(), "C_stock_torch_glue": stock_step(M),
                        "B_tracker_eager_again": lambda t=te: t.step(vs, vt)}
            tg.buffers[0].copy_(vs)
            tg.buffers[1].copy_(vt)
            st = alternate(variants, a.rounds, a.iters)
            diff = st["B_tracker_eager"]["us"] - st["C_stock_torch_glue"]["us"]
            spread = max(st[k]["max_us"] - st[k]["min_us"] for k in ("B_tracker_eager", "C_stock_torch_glue"))
            if not diff < -spread:
                missed.append("M = %d: B eager - C = %.1f us, spread %.1f us" % (M, diff, spread))
            for s in st.values():
                s["kernel_minus_stock_us"] = round(diff, 3)
                s["spread_us"] = round(spread, 3)
                s["bar_met"] = bool(diff < -spread)
                s["blind_over_tracker"] = round(st["A_blind_50000"]["us"] / st["B_tracker_eager"]["us"], 3)
            emit({"row": "ABC", "B": 1, "M": M}, st)

    if want("Q"):
        sys.path.insert(0, os.path.join(REPO))
        from tests import track_reference as tr
        P = tr.PLANTED
        for s in range(3):
            gt = tr.planted_truth(rot, s)
            Rb = T(tr.planted_init(rot, s))
            t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                      temperature=P["temperature"], batch=1, seed=s)
            track, blind = [], []
            for k in range(P["frames"]):
                tgt = ops.rotate_volume(vs, T(gt[k][None].astype(np.float32)))
                res = t.init(vs, tgt, Rb) if k == 0 else t.step(vs, tgt)
                track.append(round(float(tr.geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])), 3))
                Rp = ops.select_rotation(ops.verify_pair(vs, tgt, Rb, W1, W2, b2, want_scores=False)[1], Rb)[2][0]
                blind.append(round(float(tr.geodesic_deg(Rp.double().cpu().numpy(), gt[k])), 3))
            worst, median = tr.planted_bar(track, blind)
            rows.append(dict({"row": "Q", "sequence": s, "tracker_err_deg": track, "blind_4096_err_deg": blind,
                              "tracker_late_max_deg": round(worst, 3), "tracker_late_median_deg": round(float(np.median(track[6:])), 3),
                              "blind_median_deg": round(median, 3)}, **box))
            print(json.dumps(rows[-1]), flush=True)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if missed:
        sys.exit("bar missed (B <= C by more than the windows' spread): " + "; ".join(missed))


if __name__ == "__main__":
    main()
