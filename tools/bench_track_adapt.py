"""What adapting the noise scale on the device costs (profiles/track_adapt_step.jsonl).  The method is tools/bench_track_cv.py's:
one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max the spread), time-based
warm-up.

One pair (tests/golden/score_n128.npz), B = 1, M = 512 and 2 048 particles (sigma 3 deg, sigma_vel 1 deg, damping 1, 32 fresh
slots, T = 0.02, AdaptiveNoise() defaults: no score floor, so both trackers fill the same 32 fresh slots):
  S   PoseTracker.step for motion in (walk, constant_velocity) x (eager, captured) x (fixed, adapted): eight variants per M
      "adapted_minus_fixed_us" per (motion, mode) and "bar_us" = max(the two variants' window spread, track_advance alone);
      "bar_met" = adapted - fixed <= bar_us.  The expectation is "level": one small launch (track_control) in the place of one
      torch.ge.  Reported, met or not; the run does not fail on it.
  K   track_control alone (with and without V; score floor 0.8, n_fresh_lost M / 2), the torch.ge it replaces, track_advance alone, predict_rotations_controlled against predict_rotations and
      diffuse_rotations, at the same M
  Q   the three sequences of tests/track_adapt_reference.py on the device: per-frame errors and sigma, three seeds each

    python tools/bench_track_adapt.py [--out profiles/track_adapt_step.jsonl] [--only S,K] [--rounds 5] [--iters 200]
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

from bench_topk import alternate  # noqa: E402  (same warm-up, same windows)

SIGMA, SIGMA_VEL, DAMPING, N_FRESH, TEMP, FLOOR = 3.0, 1.0, 1.0, 32, 0.02, 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_adapt_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_track_adapt.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "sigma_deg": SIGMA, "sigma_vel_deg": SIGMA_VEL, "damping": DAMPING,
           "n_fresh": N_FRESH, "temperature": TEMP, "score_floor": FLOOR}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    R0 = T(rot.haar_rotations_np(4096, 1000))

    def tracker(M, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=SIGMA, n_fresh=N_FRESH, temperature=TEMP, batch=1, seed=0,
                                  sigma_vel_deg=SIGMA_VEL, damping=DAMPING, **kw)
        t.init(vs, vt, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(vs, vt)
        return t

    for M in (512, 2048):
        rule = lambda: ahv.track.AdaptiveNoise()
        step = torch.zeros((1,), dtype=torch.int64, device=dev)
        u = torch.empty((1,), dtype=torch.float32, device=dev)
        advance = lambda: ops.track_advance(step, 0, 1, u=u)
        adv = None
        if want("S"):
            variants, names = {}, []
            for motion in ("walk", "constant_velocity"):
                for mode, graph in (("eager", False), ("captured", True)):
                    for kind, adapt in (("fixed", None), ("adapted", rule())):
                        t = tracker(M, motion=motion, use_graph=graph, adapt=adapt)
                        if graph:
                            t.buffers[0].copy_(vs)
                            t.buffers[1].copy_(vt)
                        variants["%s_%s_%s" % (motion, mode, kind)] = (lambda t=t: t.step()) if graph else (lambda t=t: t.step(vs, vt))
                    names.append("%s_%s" % (motion, mode))
            variants["track_advance_alone"] = advance
            st = alternate(variants, a.rounds, a.iters)
            adv = st["track_advance_alone"]["us"]
            for name in names:
                f, ad = st[name + "_fixed"], st[name + "_adapted"]
                spread = max(f["max_us"] - f["min_us"], ad["max_us"] - ad["min_us"])
                diff, bar = ad["us"] - f["us"], max(spread, adv)
                for s in (f, ad):
                    s.update(adapted_minus_fixed_us=round(diff, 3), spread_us=round(spread, 3), track_advance_us=adv, bar_us=round(bar, 3),
                             bar_met=bool(diff <= bar))
            emit({"row": "S", "B": 1, "M": M}, st)
        if want("K"):
            P = T(rot.haar_rotations_np(M, 3))[None].contiguous()
            V = torch.zeros((1, M, 3), device=dev)
            idx = torch.randint(0, M, (1, M), generator=torch.Generator().manual_seed(1), dtype=torch.int64).to(dev)
            win, score = torch.full((1,), 5, dtype=torch.int64, device=dev), torch.full((1,), 0.9, device=dev)
            rec, flag = ops.track_control_state(1, SIGMA, SIGMA_VEL, N_FRESH, dev), torch.zeros((1,), dtype=torch.bool, device=dev)
            out, vel = torch.empty((1, M, 3, 3), device=dev), torch.empty((1, M, 3), device=dev)
            ckw = dict(sigma_deg=SIGMA, sigma_vel_deg=SIGMA_VEL, n_fresh=N_FRESH, score_floor=FLOOR, n_fresh_lost=M // 2, reacquired=flag)
            pkw = dict(idx=idx, step=step, seed=0, out=out)
            st = alternate({
                "track_control": lambda: ops.track_control(rec, P, win, score, **ckw),
                "track_control_with_V": lambda: ops.track_control(rec, P, win, score, V=V, first=2, **ckw),
                "torch_ge": lambda: torch.ge(win, M - N_FRESH, out=flag),
                "track_advance": advance,
                "diffuse_rotations": lambda: ops.diffuse_rotations(P, sigma_deg=SIGMA, n_fresh=N_FRESH, **pkw),
                "controlled_walk": lambda: ops.predict_rotations_controlled(P, rec, velocities=False, **pkw),
                "predict_rotations": lambda: ops.predict_rotations(P, V, sigma_deg=SIGMA, sigma_vel_deg=SIGMA_VEL, n_fresh=N_FRESH,
                                                                   vel_out=vel, **pkw),
                "controlled_cv": lambda: ops.predict_rotations_controlled(P, rec, V, vel_out=vel, **pkw),
            }, a.rounds, a.iters)
            emit({"row": "K", "B": 1, "M": M}, st)

    if want("Q"):
        from tests import track_adapt_reference as ar
        from tests import track_reference as tr
        for P, other in ((ar.ACCEL, 3.0), (ar.SETTLE, 6.0), (ar.JUMP, 3.0)):
            for s in range(3):
                Rb = T(tr.planted_init(rot, s))
                trackers = {}
                for name, sigma, adapt in (("adapted", P["sigma_deg"], ahv.track.AdaptiveNoise(**P["adapt"])), ("fixed", other, None)):
                    t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=sigma, n_fresh=P["n_fresh"],
                                              temperature=P["temperature"], batch=1, seed=s, adapt=adapt)
                    trackers[name] = (lambda tgt, t=t: t.init(vs, tgt, Rb), lambda tgt, t=t: t.step(vs, tgt),
                                      t.control if adapt is not None else None)
                err = ar.run(rot, s, P, lambda R: ops.rotate_volume(vs, T(R[None].astype(np.float32))), trackers)
                lo, hi = P["late"]
                rows.append(dict({"row": "Q", "sequence": P["name"], "s": s, "increments_deg": list(P["increments"]),
                                  "particles": P["particles"], "fixed_sigma_deg": other, "late": [lo, hi - 1],
                                  "adapted_err_deg": [round(e, 3) for e in err["adapted"][0]],
                                  "adapted_sigma_deg": [round(e, 3) for e in err["adapted"][1]],
                                  "fixed_err_deg": [round(e, 3) for e in err["fixed"][0]],
                                  "adapted_late_max_deg": round(max(err["adapted"][0][lo:hi]), 3),
                                  "adapted_late_mean_deg": round(float(np.mean(err["adapted"][0][lo:hi])), 3),
                                  "fixed_late_max_deg": round(max(err["fixed"][0][lo:hi]), 3),
                                  "fixed_late_median_deg": round(float(np.median(err["fixed"][0][lo:hi])), 3),
                                  "fixed_late_mean_deg": round(float(np.mean(err["fixed"][0][lo:hi])), 3)},
                                 **dict(box, n_fresh=P["n_fresh"], adapt=P["adapt"])))
                print(json.dumps(rows[-1]), flush=True)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
