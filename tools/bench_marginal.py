"""What marginal smoothing costs (profiles/marginal_step.jsonl).  The method is tools/bench_smooth.py's: one process, one GPU,
profiler off, the variants timed ALTERNATELY (median of the windows, min / max the spread), time-based warm-up.

One pair (tests/golden/score_n128.npz), B = 1, M = 512, 2 048, 4 096 particles (sigma 3 deg, 32 fresh slots, T = 0.02), H = 64:
  A   PoseTracker.step with history=64, eager and captured                                              (the parent's step)
  B   PoseTracker.step with history=64, marginals=True, eager and captured; "marginals_minus_history_us" = B - A for both
  C   the history=64 step followed by the forward step as the stock torch composition on the same rings: an M x M x 9
      difference tensor per frame, clamp, add, logsumexp (fp32; the slot index is a host integer here)
  K   marginal_step alone against that stock composition alone, on rings filled by the kernels
  S   marginal_smooth at F = 12 against the stock composition of the backward recursion and the finish (eleven M x M x 9
      tensors, logsumexp, log_softmax, argmax, gather)
Bar one (K and S): the kernel path is no slower than the stock composition by more than the windows' spread ("spread_us", the
wider max - min of the two rows) at every M; "bar_met" records it per M.
Bar two (A): the history-only step, which the feature touches no code of, stays within the spread of the value recorded in
profiles/smooth_step.jsonl (rows B_history_eager / B_history_captured of the same M; the spread is the wider window of the
two records, a few tenths of a microsecond for a captured step); "history_recorded_us", "history_minus_recorded_us" and
"history_bar_met" record it per M and a miss is printed.  It compares two runs, possibly on two machines: a report.
A missed bar one ends the run with exit status 1 after the rows are written.

    python tools/bench_marginal.py [--out profiles/marginal_step.jsonl] [--only K,S] [--rounds 5] [--iters 200]
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

SIGMA, N_FRESH, TEMP, H, JUMP, F = 3.0, 32, 0.02, 64, 8.0, 12


def recorded_history_step():
    """{(M, variant): row} of the history-only step in profiles/smooth_step.jsonl."""
    out = {}
    path = os.path.join(REPO, "profiles", "smooth_step.jsonl")
    if os.path.exists(path):
        for line in open(path):
            r = json.loads(line)
            if r.get("variant") in ("B_history_eager", "B_history_captured"):
                out[(r["M"], r["variant"])] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "marginal_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_marginal.py measures on the GPU only")
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
    recorded = recorded_history_step()

    def tracker(M, **kw):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=SIGMA, n_fresh=N_FRESH, temperature=TEMP, batch=1, seed=0, history=H,
                                  **kw)
        t.init(vs, vt, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(vs, vt)
        return t

    def stock_w(P, R, M):
        diff = P.reshape(1, M, 1, 9) - R.reshape(1, 1, M, 9)
        return (-(diff * diff).sum(-1) * k4).clamp_(min=-JUMP)

    def stock_forward(hist, marg, R, s, t):
        """The stock fp32 torch composition of one forward step into ``marg``; t is a host integer."""
        M = R.shape[1]
        prev, slot = (t - 1) % H, t % H
        al = marg.alpha[prev]
        lse = torch.logsumexp((al - al.max(dim=1, keepdim=True).values)[:, :, None] + stock_w(hist.R[prev], R, M), dim=1)
        torch.mul(s, beta, out=marg.emit[slot])
        torch.add(marg.emit[slot], lse, out=marg.alpha[slot])

    def stock_smooth(hist, marg, t, out):
        """The stock fp32 torch composition of the backward recursion and the finish over the newest F frames."""
        M = hist.R.shape[2]
        bt = torch.zeros_like(marg.alpha[0])
        for back in range(F):
            slot = (t - back) % H
            lw = torch.log_softmax(marg.alpha[slot] + bt, dim=1)
            out.logw[:, F - 1 - back] = lw
            idx = lw.argmax(dim=1)
            out.idx[:, F - 1 - back] = idx
            out.R[:, F - 1 - back] = hist.R[slot][torch.arange(idx.shape[0], device=idx.device), idx]
            if back + 1 < F:
                gj = marg.emit[slot] + bt
                gj = gj - gj.max(dim=1, keepdim=True).values
                bt = torch.logsumexp(stock_w(hist.R[(t - back - 1) % H], hist.R[slot], M) + gj[:, None, :], dim=2)

    def bar_one(st, kernel, stock, M, what, missed):
        diff = st[kernel]["us"] - st[stock]["us"]
        spread = max(v["max_us"] - v["min_us"] for v in st.values())
        if not diff <= spread:
            missed.append("%s, M = %d: kernel - stock = %.1f us, spread %.1f us" % (what, M, diff, spread))
        for v in st.values():
            v["kernel_minus_stock_us"], v["spread_us"], v["bar_met"] = round(diff, 3), round(spread, 3), bool(diff <= spread)

    missed, drifted = [], []
    for M in (512, 2048, 4096):
        if want("A") or want("B") or want("C"):
            he, hg, me, mgr, ce = (tracker(M), tracker(M, use_graph=True), tracker(M, marginals=True),
                                   tracker(M, marginals=True, use_graph=True), tracker(M))
            marg = ops.marginal_history(1, M, H, dev)
            for x in marg:
                x.zero_()
            count = [3]

            def stock_step():
                o = ce.step(vs, vt)
                count[0] += 1
                stock_forward(ce._hist, marg, o.particles, o.scores, count[0])

            variants = {"A_history_eager": lambda t=he: t.step(vs, vt), "A_history_captured": lambda t=hg: t.step(),
                        "B_marginals_eager": lambda t=me: t.step(vs, vt), "B_marginals_captured": lambda t=mgr: t.step(),
                        "C_stock_torch_forward": stock_step}
            for t in (hg, mgr):
                t.buffers[0].copy_(vs)
                t.buffers[1].copy_(vt)
            st = alternate(variants, a.rounds, a.iters)
            for s in st.values():
                s["marginals_minus_history_us"] = round(st["B_marginals_eager"]["us"] - st["A_history_eager"]["us"], 3)
                s["marginals_minus_history_captured_us"] = round(st["B_marginals_captured"]["us"] - st["A_history_captured"]["us"], 3)
                s["stock_minus_history_us"] = round(st["C_stock_torch_forward"]["us"] - st["A_history_eager"]["us"], 3)
            for name, old in (("A_history_eager", "B_history_eager"), ("A_history_captured", "B_history_captured")):
                rec = recorded.get((M, old))
                if rec is None:
                    continue
                s = st[name]
                diff = s["us"] - rec["us"]
                spread = max(s["max_us"] - s["min_us"], rec["max_us"] - rec["min_us"])
                s["history_recorded_us"], s["history_minus_recorded_us"] = rec["us"], round(diff, 3)
                s["history_spread_us"], s["history_bar_met"] = round(spread, 3), bool(abs(diff) <= spread)
                if not abs(diff) <= spread:
                    drifted.append("%s, M = %d: %.1f us now, %.1f us recorded, spread %.1f us" % (name, M, s["us"], rec["us"], spread))
            emit({"row": "ABC", "B": 1, "M": M}, st)
        if want("K") or want("S"):
            R = [ops.random_rotations(M, seed=5 + f, device=dev)[None].contiguous() for f in range(2)]
            s = [torch.rand(1, M, device=dev) * 2 - 1 for f in range(2)]
            hist, mk, ms = ops.smooth_history(1, M, H, dev), ops.marginal_history(1, M, H, dev), ops.marginal_history(1, M, H, dev)
            for f in range(F + 1):       # slots 1..F+1 hold frames: the timed step is frame F + 2, with predecessors
                step = torch.full((1,), f + 1, dtype=torch.int64, device=dev)
                ops.smooth_step(hist, R[f & 1], s[f & 1], step, TEMP, SIGMA, jump=JUMP)
                ops.marginal_step(hist, mk, R[f & 1], s[f & 1], step, TEMP, SIGMA, jump=JUMP)
            for x, y in zip(ms, mk):
                x.copy_(y)
            last = F + 1
            nxt = torch.full((1,), last + 1, dtype=torch.int64, device=dev)
            if want("K"):
                st = alternate({"K_marginal_step_kernel": lambda: ops.marginal_step(hist, mk, R[0], s[0], nxt, TEMP, SIGMA, jump=JUMP),
                                "K_stock_torch_composition": lambda: stock_forward(hist, ms, R[0], s[0], last + 1)}, a.rounds, a.iters)
                torch.cuda.synchronize()
                err = float((mk.alpha[(last + 1) % H] - ms.alpha[(last + 1) % H]).abs().max())
                bar_one(st, "K_marginal_step_kernel", "K_stock_torch_composition", M, "marginal_step", missed)
                for v in st.values():
                    v["max_abs_alpha_difference"] = err
                emit({"row": "K", "B": 1, "M": M}, st)
            if want("S"):
                cur = torch.full((1,), last, dtype=torch.int64, device=dev)
                ok = ops.marginal_smooth(hist, mk, cur, SIGMA, jump=JUMP, frames=F)
                os_ = ops.SmoothedMarginals(*[torch.zeros_like(x) for x in ok])
                st = alternate({"S_marginal_smooth_kernels": lambda: ops.marginal_smooth(hist, mk, cur, SIGMA, jump=JUMP, frames=F, out=ok),
                                "S_stock_torch_composition": lambda: stock_smooth(hist, mk, last, os_)}, a.rounds, max(a.iters // 10, 10))
                torch.cuda.synchronize()
                err = float((ok.logw - os_.logw).abs().max())
                bar_one(st, "S_marginal_smooth_kernels", "S_stock_torch_composition", M, "marginal_smooth", missed)
                for v in st.values():
                    v["max_abs_log_gamma_difference"], v["frames"] = err, F
                    v["same_argmax"] = bool(torch.equal(ok.idx, os_.idx))
                emit({"row": "S", "B": 1, "M": M}, st)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if drifted:
        print("bar two (the history-only step against its record) missed: " + "; ".join(drifted), file=sys.stderr)
    if missed:
        sys.exit("bar one missed (kernel path no slower than the stock composition by more than the spread): " + "; ".join(missed))


if __name__ == "__main__":
    main()
