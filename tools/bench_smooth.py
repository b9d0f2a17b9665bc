"""What trajectory smoothing costs, and what it buys (profiles/smooth_step.jsonl).  The method is tools/bench_track.py's: one
process, one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max the spread), time-based warm-up.

One pair (tests/golden/score_n128.npz), B = 1, M = 512, 2 048, 4 096 particles (sigma 3 deg, 32 fresh slots, T = 0.02), H = 64:
  A   PoseTracker.step with history=0, eager and captured                                                  (the parent's step)
  B   PoseTracker.step with history=64, eager and captured; "history_minus_plain_us" = B - A for both: reported, not barred
  C   the history=0 step followed by the smoothing step as the stock torch composition on the same ring buffers: an M x M x 9
      difference tensor per frame, clamp, add, max (fp32; the slot index is a host integer here, which the kernel reads on
      the device)
  K   smooth_step alone against that stock composition alone, on a ring filled by the kernel.  The bar: the kernel is faster
      by more than the windows' spread ("spread_us", the wider max - min of the two rows) at every M; "bar_met" records it
      per M, and a missed bar ends the run with exit status 1 after the rows are written.
  T   smooth_backtrace at F = 64 and F = 256 (M = 512, H = 256): a chain of F dependent loads.
  Q   the planted sequence with two distractor frames of tests/smooth_reference.py on the device, smooth_jump 8 and 4, and the
      clean sequence: per-frame errors of the filter and of the smoothed path, three sequences.  Reported without a bar
      (tests/test_gpu_smooth.py holds the bar).

    python tools/bench_smooth.py [--out profiles/smooth_step.jsonl] [--only K,Q] [--rounds 5] [--iters 200]
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

SIGMA, N_FRESH, TEMP, H, JUMP = 3.0, 32, 0.02, 64, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smooth_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_smooth.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "sigma_deg": SIGMA, "n_fresh": N_FRESH, "temperature": TEMP, "H": H, "jump": JUMP}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    beta = ops.inverse_temperature(TEMP)
    k4 = 1.0 / (4.0 * ops._angle_rad(SIGMA, "sigma_deg") ** 2)
    R0 = T(rot.haar_rotations_np(4096, 1000))

    def tracker(M, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=SIGMA, n_fresh=N_FRESH, temperature=TEMP, batch=1, seed=0, **kw)
        t.init(vs, vt, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(vs, vt)
        return t

    def stock_smooth(hist, R, s, t):
        """The stock fp32 torch composition of one smoothing step into the ring ``hist``; t is a host integer."""
        M = R.shape[1]
        prev, slot = (t - 1) % H, t % H
        d = hist.delta[prev]
        diff = hist.R[prev].reshape(1, M, 1, 9) - R.reshape(1, 1, M, 9)
        w = (-(diff * diff).sum(-1) * k4).clamp_(min=-JUMP)
        best, idx = ((d - d.max(dim=1, keepdim=True).values)[:, :, None] + w).max(dim=1)
        hist.R[slot].copy_(R)
        torch.add(s * beta, best, out=hist.delta[slot])
        hist.back[slot].copy_(idx)

    missed = []
    for M in (512, 2048, 4096):
        if want("A") or want("B") or want("C"):
            pe, pg, he, hg, ce = (tracker(M), tracker(M, use_graph=True), tracker(M, history=H), tracker(M, history=H, use_graph=True),
                                  tracker(M))
            ring = ops.smooth_history(1, M, H, dev)
            for x in (ring.R, ring.delta):
                x.zero_()
            count = [3]

            def stock_step():
                o = ce.step(vs, vt)
                count[0] += 1
                stock_smooth(ring, o.particles, o.scores, count[0])

            variants = {"A_plain_eager": lambda t=pe: t.step(vs, vt), "A_plain_captured": lambda t=pg: t.step(),
                        "B_history_eager": lambda t=he: t.step(vs, vt), "B_history_captured": lambda t=hg: t.step(),
                        "C_stock_torch_smoothing": stock_step}
            for t in (pg, hg):
                t.buffers[0].copy_(vs)
                t.buffers[1].copy_(vt)
            st = alternate(variants, a.rounds, a.iters)
            for s in st.values():
                s["history_minus_plain_us"] = round(st["B_history_eager"]["us"] - st["A_plain_eager"]["us"], 3)
                s["history_minus_plain_captured_us"] = round(st["B_history_captured"]["us"] - st["A_plain_captured"]["us"], 3)
                s["stock_minus_plain_us"] = round(st["C_stock_torch_smoothing"]["us"] - st["A_plain_eager"]["us"], 3)
            emit({"row": "ABC", "B": 1, "M": M}, st)
        if want("K"):
            R = [ops.random_rotations(M, seed=5 + f, device=dev)[None].contiguous() for f in range(2)]
            s = [torch.rand(1, M, device=dev) * 2 - 1 for f in range(2)]
            hk, hs = ops.smooth_history(1, M, H, dev), ops.smooth_history(1, M, H, dev)
            for f in range(4):          # slots 1..4 hold frames: the timed step is frame 5, with predecessors
                ops.smooth_step(hk, R[f & 1], s[f & 1], torch.full((1,), f + 1, dtype=torch.int64, device=dev), TEMP, SIGMA, jump=JUMP)
            for x, y in zip(hs, hk):
                if x is not None:
                    x.copy_(y)
            five = torch.full((1,), 5, dtype=torch.int64, device=dev)
            st = alternate({"K_smooth_step_kernel": lambda: ops.smooth_step(hk, R[0], s[0], five, TEMP, SIGMA, jump=JUMP),
                            "K_stock_torch_composition": lambda: stock_smooth(hs, R[0], s[0], 5)}, a.rounds, a.iters)
            torch.cuda.synchronize()
            err = float((hk.delta[5] - hs.delta[5]).abs().max())
            diff = st["K_smooth_step_kernel"]["us"] - st["K_stock_torch_composition"]["us"]
            spread = max(v["max_us"] - v["min_us"] for v in st.values())
            if not diff < -spread:
                missed.append("M = %d: kernel - stock = %.1f us, spread %.1f us" % (M, diff, spread))
            for v in st.values():
                v["kernel_minus_stock_us"], v["spread_us"], v["bar_met"] = round(diff, 3), round(spread, 3), bool(diff < -spread)
                v["max_abs_delta_difference"] = err
            emit({"row": "K", "B": 1, "M": M}, st)

    if want("T"):
        M, HT = 512, 256
        hist = ops.smooth_history(1, M, HT, dev)
        step = torch.zeros((1,), dtype=torch.int64, device=dev)
        for f in range(HT):
            step += 1
            ops.smooth_step(hist, ops.random_rotations(M, seed=f, device=dev)[None].contiguous(), torch.rand(1, M, device=dev), step, TEMP,
                            SIGMA, jump=JUMP)
        outs = {F: ops.smooth_backtrace(hist, step, frames=F) for F in (64, 256)}
        st = alternate({"T_backtrace_F%d" % F: (lambda F=F: ops.smooth_backtrace(hist, step, frames=F, out=outs[F])) for F in (64, 256)},
                       a.rounds, a.iters)
        emit({"row": "T", "B": 1, "M": M, "H_ring": HT}, st)

    if want("Q"):
        from tests import smooth_reference as sm
        from tests import track_reference as tr
        P = sm.DISTRACTED
        rotate = lambda R: ops.rotate_volume(vs, T(R[None].astype(np.float32)))
        for s in range(3):
            Rb = T(tr.planted_init(rot, s))
            gt = tr.planted_truth(rot, s)

            def make(jump):
                return ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                             temperature=P["temperature"], batch=1, seed=s, history=P["history"],
                                             smooth_sigma_deg=P["smooth_sigma_deg"], smooth_jump=jump)

            row = {"row": "Q", "sequence": s, "particles": P["particles"], "history": P["history"], "smooth_sigma_deg": P["smooth_sigma_deg"]}
            for jump in (8.0, 4.0):
                t = make(jump)
                filt, smooth = sm.distracted_run(rot, s, rotate, lambda v: t.init(vs, v, Rb), lambda v: t.step(vs, v), t.smoothed)
                row["distracted_filter_err_deg"] = [round(float(e), 3) for e in filt]
                row["distracted_smoothed_err_deg_jump%g" % jump] = [round(float(e), 3) for e in smooth]
            t = make(8.0)
            clean = []
            for k in range(P["frames"]):
                res = t.init(vs, rotate(gt[k]), Rb) if k == 0 else t.step(vs, rotate(gt[k]))
                clean.append(float(tr.geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])))
            cs = tr.geodesic_deg(t.smoothed().R[0].double().cpu().numpy(), gt[1:])
            row["clean_filter_err_deg"] = [round(e, 3) for e in clean]
            row["clean_smoothed_err_deg"] = [round(float(e), 3) for e in cs]
            row["clean_filter_mean_deg"], row["clean_smoothed_mean_deg"] = round(float(np.mean(clean[1:])), 3), round(float(np.mean(cs)), 3)
            rows.append(dict(row, **dict(box, H=P["history"])))
            print(json.dumps(rows[-1]), flush=True)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if missed:
        sys.exit("bar missed (kernel <= stock by more than the windows' spread): " + "; ".join(missed))


if __name__ == "__main__":
    main()
