"""What the constant-velocity predict step costs, and what it buys (profiles/track_cv_step.jsonl).  The method is
tools/bench_track.py's: one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max the
spread), time-based warm-up.

One pair (tests/golden/score_n128.npz), B = 1, M = 512, 2 048, 4 096 particles (sigma 3 deg, sigma_vel 1 deg, damping 1, 32 fresh
slots, T = 0.02):
  W   PoseTracker.step with motion="walk", eager and captured                                             (the parent's code path)
  V   PoseTracker.step with motion="constant_velocity", eager and captured
  C   the constant-velocity step with its glue in stock torch around the same scorer launch: softmax / cumsum / searchsorted
      for the draws, torch.randn for both noises, indexing for the velocities, axis_angle_to_matrix + matmul for the move
      (fp32; its draws and noise are NOT the kernels' bit for bit), the elite, the coast slot and the fresh slots by indexing
      "kernel_minus_stock_us" = V eager - C; the bar: negative by more than the windows' spread ("spread_us", the widest
      max - min of the two rows) at every M.  "bar_met" records it per M, and a missed bar ends the run with exit status 1
      after the rows are written.
      "cv_minus_walk_us" = V eager - W eager (and "cv_minus_walk_captured_us"), with "level" true when it is inside the spread
      of those rows: reported, not barred -- the step is launch-bound, and the expectation is "level".
  Q   the fast planted sequence of tests/track_cv_reference.py on the device (9 degrees per frame): per-frame errors of both
      trackers, three sequences.  Reported without a bar (tests/test_gpu_track_cv.py holds the bar).

    python tools/bench_track_cv.py [--out profiles/track_cv_step.jsonl] [--only W,Q] [--rounds 5] [--iters 200]
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

SIGMA, SIGMA_VEL, DAMPING, N_FRESH, TEMP = 3.0, 1.0, 1.0, 32, 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_cv_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_track_cv.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "sigma_deg": SIGMA, "sigma_vel_deg": SIGMA_VEL, "damping": DAMPING,
           "n_fresh": N_FRESH, "temperature": TEMP}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    beta = ops.inverse_temperature(TEMP)
    R0 = T(rot.haar_rotations_np(4096, 1000))

    def tracker(M, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=SIGMA, n_fresh=N_FRESH, temperature=TEMP, batch=1, seed=0,
                                  sigma_vel_deg=SIGMA_VEL, damping=DAMPING, **kw)
        t.init(vs, vt, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(vs, vt)
        return t

    def stock_step(M):
        """The constant-velocity step's glue in stock torch; the scorer launch and select_rotation are the tracker's."""
        state = {"R": R0[None].expand(1, -1, -1, -1).contiguous(), "V": torch.zeros(1, R0.shape[0], 3, device=dev),
                 "s": ops.verify_pair(vs, vt, R0, W1, W2, b2)[0], "best": torch.zeros(1, dtype=torch.int64, device=dev)}
        key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)
        ar = (torch.arange(M, device=dev, dtype=torch.float32))[None]
        sig, sig_v = math.radians(SIGMA), math.radians(SIGMA_VEL)

        def f():
            R, V, s = state["R"], state["V"], state["s"]
            u = torch.rand(1, 1, device=dev)
            c = torch.cumsum(torch.softmax(s * beta, dim=1), dim=1)
            idx = torch.searchsorted(c, ((ar + u) / M).contiguous(), right=True).clamp_(max=s.shape[1] - 1)
            vel = DAMPING * V[0][idx[0]] + torch.randn(M, 3, device=dev) * sig_v
            w = vel + torch.randn(M, 3, device=dev) * sig
            new = torch.matmul(R[0][idx[0]], rot.axis_angle_to_matrix(w))[None]
            vel = vel[None]
            v_best = V[0][state["best"]]
            new[:, 0] = R[0][state["best"]]
            new[:, 1] = torch.matmul(R[0][state["best"]], rot.axis_angle_to_matrix(v_best))
            vel[:, 0] = v_best
            vel[:, 1] = v_best
            new[:, M - N_FRESH:] = rot.random_rotations(N_FRESH, device=dev)[None]
            vel[:, M - N_FRESH:] = 0.0
            new = new.contiguous()
            s2, _ = ops.verify_pair(vs, vt, new, W1, W2, b2, want_scores=True, best_key=key, reset_best=True)
            sc, i, Rm = ops.select_rotation(key, new)
            state["R"], state["V"], state["s"], state["best"] = new, vel, s2, i
            return sc, i, Rm
        return f

    missed = []
    if want("W") or want("V") or want("C"):
        for M in (512, 2048, 4096):
            cv = dict(motion="constant_velocity")
            we, wg, ve, vg = tracker(M), tracker(M, use_graph=True), tracker(M, **cv), tracker(M, use_graph=True, **cv)
            variants = {"W_walk_eager": lambda t=we: t.step(vs, vt), "W_walk_captured": lambda t=wg: t.step(),
                        "V_cv_eager": lambda t=ve: t.step(vs, vt), "V_cv_captured": lambda t=vg: t.step(),
                        "C_stock_torch_glue": stock_step(M), "V_cv_eager_again": lambda t=ve: t.step(vs, vt)}
            for t in (wg, vg):
                t.buffers[0].copy_(vs)
                t.buffers[1].copy_(vt)
            st = alternate(variants, a.rounds, a.iters)
            width = lambda *names: max(st[k]["max_us"] - st[k]["min_us"] for k in names)
            diff = st["V_cv_eager"]["us"] - st["C_stock_torch_glue"]["us"]
            spread = width("V_cv_eager", "C_stock_torch_glue")
            if not diff < -spread:
                missed.append("M = %d: V eager - C = %.1f us, spread %.1f us" % (M, diff, spread))
            d_e = st["V_cv_eager"]["us"] - st["W_walk_eager"]["us"]
            d_g = st["V_cv_captured"]["us"] - st["W_walk_captured"]["us"]
            level = abs(d_e) <= width("V_cv_eager", "W_walk_eager") and abs(d_g) <= width("V_cv_captured", "W_walk_captured")
            for s in st.values():
                s["kernel_minus_stock_us"] = round(diff, 3)
                s["spread_us"] = round(spread, 3)
                s["bar_met"] = bool(diff < -spread)
                s["cv_minus_walk_us"] = round(d_e, 3)
                s["cv_minus_walk_captured_us"] = round(d_g, 3)
                s["walk_spread_us"] = round(width("V_cv_eager", "W_walk_eager"), 3)
                s["walk_spread_captured_us"] = round(width("V_cv_captured", "W_walk_captured"), 3)
                s["level"] = bool(level)
            emit({"row": "WVC", "B": 1, "M": M}, st)

    if want("Q"):
        from tests import track_cv_reference as cvr
        from tests import track_reference as tr
        P = cvr.FAST
        for s in range(3):
            Rb = T(tr.planted_init(rot, s))
            trackers = {}
            for motion in ("walk", "constant_velocity"):
                t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                          temperature=P["temperature"], batch=1, seed=s, motion=motion,
                                          sigma_vel_deg=P["sigma_vel_deg"], damping=P["damping"])
                trackers[motion] = (lambda tgt, t=t: t.init(vs, tgt, Rb), lambda tgt, t=t: t.step(vs, tgt))
            err = cvr.run(rot, s, P, lambda R: ops.rotate_volume(vs, T(R[None].astype(np.float32))), trackers)
            worst, median = cvr.fast_bar(err["constant_velocity"], err["walk"])
            rows.append(dict({"row": "Q", "sequence": s, "deg_per_frame": P["deg_per_frame"], "particles": P["particles"],
                              "walk_err_deg": [round(e, 3) for e in err["walk"]],
                              "cv_err_deg": [round(e, 3) for e in err["constant_velocity"]],
                              "cv_late_max_deg": round(worst, 3), "walk_late_median_deg": round(median, 3)},
                             **dict(box, n_fresh=P["n_fresh"])))
            print(json.dumps(rows[-1]), flush=True)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if missed:
        sys.exit("bar missed (V <= C by more than the windows' spread): " + "; ".join(missed))


if __name__ == "__main__":
    main()
