"""What the multi-view fusion costs (profiles/views_step.jsonl).  The method is tools/bench_modes.py's: one process, one GPU,
profiler off, the variants timed ALTERNATELY (median of the rounds, min / max the spread), time-based warm-up.

One query x 50 000 hypotheses of its rotation, V = 4 and V = 8 posed reference views:
  A   what a user can do without the fusion: forward_3d2d(query), Q A^T as one plain GEMM, score_hypotheses over the V
      samples, then ops.argmax per view -- V unrelated arg-maxes (timed twice: A and A2 give the spread)
  B   ops.verify_views (view_rotations + one scoring launch + fuse_view_scores) then select_rotation; B_key: the same without
      the fused row written
  C   B's scoring launch with the glue in stock torch: Q @ A.mT (a batched 3 x 3 matmul), mean(0), torch.max, gather
  C2  C with the composition as ONE plain GEMM (3 N x 3) @ (3 x 3 V) + a permuting copy: the cheapest stock form
"added_us_over_A" = the variant minus A; "B_minus_C_us" / "B_minus_C2_us" on the B rows.

    python tools/bench_views.py [--out profiles/views_step.jsonl] [--rounds 5] [--iters 100]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "views_step.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--n", type=int, default=50_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_views.py measures on the GPU only")
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

        def compose_gemm():   # Q_n A_v^T as ONE plain GEMM (3 N x 3) @ (3 x 3 V): the cheap stock form
            return (Q.reshape(N * 3, 3) @ A[0].reshape(V * 3, 3).T).reshape(N, 3, V, 3).permute(2, 0, 1, 3).contiguous()

        def step_a():
            ft = ops.forward_3d2d(query, W1, W2, b2).expand(V, -1, -1)
            Rv = compose_gemm()
            s, _ = ops.score_hypotheses(refs[0], ft, Rv, W1, W2, b2)
            return ops.argmax(s)

        def step_b(want_scores):
            def f():
                _, k = ops.verify_views(refs, query, Q, A, W1, W2, b2, want_scores=want_scores, best_key=key, reset_best=True)
                return ops.select_rotation(k, Q)
            return f

        def step_c(compose):
            def f():
                s, _ = ops.verify_pair(refs[0], query.expand(V, -1, -1, -1, -1), compose(), W1, W2, b2)
                val, idx = torch.max(s.mean(0, keepdim=True), dim=1)
                return val, idx, Q[idx]
            return f

        _, idx_b, _ = step_b(True)()
        _, idx_c, _ = step_c(lambda: torch.matmul(Q[None], A[0].mT[:, None]))()
        _, idx_c2, _ = step_c(compose_gemm)()
        assert torch.equal(idx_c, idx_c2)
        variants = {"A_score_hypotheses_argmax_per_view": step_a, "A2_same_again": step_a,
                    "B_verify_views_select_rotation": step_b(True), "B_key_only": step_b(False),
                    "C_scorer_torch_glue": step_c(lambda: torch.matmul(Q[None], A[0].mT[:, None])),
                    "C2_scorer_torch_glue_gemm_compose": step_c(compose_gemm)}
        st = alternate(variants, a.rounds, a.iters)
        base, c = st["A_score_hypotheses_argmax_per_view"]["us"], st["C_scorer_torch_glue"]["us"]
        c2 = st["C2_scorer_torch_glue_gemm_compose"]["us"]
        for name, s in st.items():
            s["added_us_over_A"] = round(s["us"] - base, 3)
            if name.startswith("B_"):
                s["B_minus_C_us"] = round(s["us"] - c, 3)
                s["B_minus_C2_us"] = round(s["us"] - c2, 3)
                s["same_index_as_C"] = bool(torch.equal(idx_b, idx_c))
            rows.append(dict({"row": "ABC", "B": 1, "V": V, "N": N}, variant=name, **s, **box))
            print(json.dumps(rows[-1]), flush=True)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
