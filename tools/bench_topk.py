"""What the K-best selection costs (profiles/topk_step.jsonl).  One process, one GPU, profiler off; every row of a run shares
the box and the clock state, and the variants are timed ALTERNATELY over several rounds (the median of the rounds is the
figure, min / max the spread).

  A   verify_pair + select_rotation, B = 1 x 50 000: the step as it was (timed twice: A and A2 give the spread)
  B   verify_pair_topk (K = 16, 64) + select_topk: A plus the feature; "added_us" = B - A
  C   the stock composition: verify_pair(want_scores=True) + torch.topk + index gather
  D   ahv_topk_f32 alone at B = 32 x 50 000 (6.4 MB of scores), K = 16: event time here; the kernel times come from a
      `rocprofv3 --kernel-trace --stats -- python tools/bench_topk.py --only D` run of its own
  E   CoarseToFine 10 000 + 1 000 with seeds = 1, 4, 8, eager and captured

    python tools/bench_topk.py [--out profiles/topk_step.jsonl] [--only D] [--rounds 5] [--iters 200]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def warm(fns, warm_ms=120.0, least=5):
    """Time-based warm-up past the ~30 ms clock ramp after an idle period, every shape of the timed window included."""
    t0, n = time.perf_counter(), 0
    while n < least or (time.perf_counter() - t0) * 1e3 < warm_ms:
        for f in fns:
            f()
        torch.cuda.synchronize()
        n += 1


def window(fn, iters):
    """us per call between two device events around ``iters`` launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(variants, rounds, iters):
    """{name: fn} -> {name: {"us": median, "min_us", "max_us", "rounds"}}, the variants taking turns inside every round."""
    warm(list(variants.values()))
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            got[k].append(window(f, iters))
    return {k: {"us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "rounds": rounds, "iters": iters} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_topk.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops = ahv.ops
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    gb = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    N = 50_000
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(N, 7)).to(dev)
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count()}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")

    if want("A") or want("B") or want("C"):
        key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

        def step_a():
            ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=False, best_key=key, reset_best=False)
            return ops.select_rotation(key, R, reset_key=True)

        # B and C reset the arg-max key with a launch of their own (reset_best=True) while A's select hands it back empty:
        # a small bias against B and C alike, none between them
        def step_b(k):
            klist = torch.empty((1, k), dtype=torch.int64, device=dev)

            def f():
                ops.verify_pair_topk(vs, vt, R, W1, W2, b2, k, keys=klist, reset=True, best_key=key, reset_best=True)
                return ops.select_topk(klist, R)
            return f

        def step_c(k):
            def f():
                s, _ = ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True, best_key=key, reset_best=True)
                val, idx = torch.topk(s, k, dim=1)
                return val, idx, R[idx]
            return f

        variants = {"A_verify_pair_select_rotation": step_a, "A2_same_again": step_a}
        for k in (16, 64):
            variants["B_verify_pair_topk_select_topk_K%d" % k] = step_b(k)
            variants["C_verify_pair_torch_topk_gather_K%d" % k] = step_c(k)
        # same answer first: the stock composition's values are the list's (its index order among ties is unspecified)
        for k in (16, 64):
            sc, idx, _ = variants["B_verify_pair_topk_select_topk_K%d" % k]()
            val, _, _ = variants["C_verify_pair_torch_topk_gather_K%d" % k]()
            assert torch.equal(sc, val), "top-%d values differ from torch.topk" % k
        st = alternate(variants, a.rounds, a.iters)
        base = st["A_verify_pair_select_rotation"]["us"]
        for name, s in st.items():
            s["added_us_over_A"] = round(s["us"] - base, 3)
        emit({"row": "ABC", "B": 1, "N": N}, st)

    if want("D"):
        B, K = 32, 16
        s = torch.randn(B, N, device=dev)
        klist = torch.empty((B, K), dtype=torch.int64, device=dev)
        st = alternate({"D_topk_B32_K16": lambda: ops.topk(s, K, keys=klist, reset=True),
                        "D_torch_topk_B32_K16": lambda: torch.topk(s, K, dim=1)}, a.rounds, a.iters)
        for v in st.values():
            v["score_bytes"] = 4 * B * N
            v["GBps_event_time"] = round(4 * B * N / (v["us"] * 1e-6) / 1e9, 1)
        emit({"row": "D", "B": B, "N": N, "K": K}, st)

    if want("E"):
        vs3, vt3 = T(gb["vol_src"][:1]), T(gb["vol_tgt"][:1])
        Rc = torch.from_numpy(ahv.rotations.haar_rotations_np(10_000, 40)).to(dev)
        variants = {}
        for seeds in (1, 4, 8):
            for graph in (False, True):
                c2f = ahv.refine.CoarseToFine(W1, W2, b2, Rc, n_fine=1000, batch=1, use_graph=graph, seeds=seeds)
                c2f(vs3, vt3)
                variants["E_seeds%d_%s_fine%d" % (seeds, "graph" if graph else "eager", seeds * 1000)] = \
                    (lambda c=c2f: c(vs3, vt3)) if not graph else (lambda c=c2f: c())
        emit({"row": "E", "B": 1, "N_coarse": 10_000, "N_fine_per_seed": 1000}, alternate(variants, a.rounds, a.iters))

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
