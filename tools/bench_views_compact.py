"""What the angle limit saves when only the participating pairs are scored (profiles/views_compact_step.jsonl).  The method is
tools/bench_views.py's: one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the rounds, min / max the
spread), time-based warm-up.

One query x 50 000 Haar hypotheses of its rotation, V = 4 and V = 8 posed reference views, theta = 60, 90 and 150 degrees
(Haar share of participating pairs 0.058, 0.182, 0.674):
  dense         ops.verify_views with the limit (every pair composed and scored, the limit applied in the fuse) + select_rotation
  compact_sync  the same with compact=True, capacity=None: a count-only call, ONE host read of the largest count, then the step
  compact_cap   compact=True with capacity = N p + 6 sqrt(N p (1 - p)), p = ops.haar_view_fraction(theta): no host read
  dense_at_M_sync / dense_at_M_cap   the dense step on the first M hypotheses, M = what compact_sync / compact_cap scores per view:
                the same scorer work without the compaction.  "glue_us" on the compact rows = the row minus its dense_at_M -- the
                two compaction launches (twice the count kernel and the host read for compact_sync) and the slot map.
Each compact row records counts, M and whether its index equals the dense one; "saved_us" = dense minus the row, and
"clear_of_spread" says whether the slowest compact round still beats the fastest dense round.

    python tools/bench_views_compact.py [--out profiles/views_compact_step.jsonl] [--rounds 5] [--iters 100]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "views_compact_step.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--n", type=int, default=50_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_views_compact.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops = ahv.ops
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    obj, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "W1", "W2", "b2"))
    N = a.n
    Q = T(ahv.rotations.haar_rotations_np(N, 7))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count()}
    rows = []
    for V in (4, 8):
        A = T(ahv.rotations.haar_rotations_np(V, 70 + V))[None]                     # (1,V,3,3)
        refs = ops.rotate_volume(obj.expand(V, -1, -1, -1, -1), A[0])[None]          # (1,V,16,8,8,8)
        query = ops.rotate_volume(obj, Q[4321:4322])
        key = torch.empty((1,), dtype=torch.int64, device=dev)
        for theta in (60.0, 90.0, 150.0):
            p = ops.haar_view_fraction(theta)
            cap = min(N, int(math.ceil(N * p + 6.0 * math.sqrt(N * p * (1.0 - p)))))
            counts = ops.view_rotations_compact(Q, A, theta)[2]
            m_sync = max(1, int(counts.max()))

            def step(Qs, **kw):
                def f():
                    _, k = ops.verify_views(refs, query, Qs, A, W1, W2, b2, max_view_angle_deg=theta, best_key=key,
                                            reset_best=True, **kw)
                    return ops.select_rotation(k, Qs)
                return f

            variants = {"dense": step(Q), "compact_sync": step(Q, compact=True), "compact_cap": step(Q, compact=True, capacity=cap),
                        "dense_at_M_sync": step(Q[:m_sync].contiguous()), "dense_at_M_cap": step(Q[:cap].contiguous())}
            idx = {k: int(f()[1].item()) for k, f in variants.items()}
            st = alternate(variants, a.rounds, a.iters)
            dense = st["dense"]
            for name, s in st.items():
                s["predicted_share_of_dense"] = round(p, 4)
                if name.startswith("compact"):
                    m = m_sync if name == "compact_sync" else cap
                    at_m = st["dense_at_M_sync" if name == "compact_sync" else "dense_at_M_cap"]
                    s.update(M=m, counts=counts[0].tolist(), overflow=bool(m < m_sync), same_index_as_dense=idx[name] == idx["dense"],
                             glue_us=round(s["us"] - at_m["us"], 3), saved_us=round(dense["us"] - s["us"], 3),
                             share_of_dense=round(s["us"] / dense["us"], 4), clear_of_spread=bool(s["max_us"] < dense["min_us"]))
                rows.append(dict({"row": "compact", "B": 1, "V": V, "N": N, "theta_deg": theta}, variant=name, **s, **box))
                print(json.dumps(rows[-1]), flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
