"""What a tracker step against several posed reference views costs (profiles/track_views_step.jsonl).  The method is
tools/bench_track.py's: one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max the
spread), time-based warm-up.

The plant of tests/track_views_reference.py (V = 8 views 45 degrees apart, 60 degrees, sigma 3 degrees, 32 fresh slots, T = 0.02),
B = 1, a fixed frame 10 degrees into the turn, M = 512 and 2 048:
  S   the single-reference step (``views=None``), eager and captured: the parent's calls; compare with profiles/track_step.jsonl
  V   PoseTracker(views=A).step(refs (1,V,...), query) at K = 2 and K = 8, eager and captured
  D   baseline 2, what a user could compose before: the same filter with ``ops.verify_views`` over all V views as its scoring call
      (track_advance, resample, diffuse_rotations, verify_views, select_rotation)
  T   baseline 3, the K = 2 step with selection and gather in stock torch: traces by einsum, argsort, index_select / expand,
      then the same chain (verify_views_staged with its workspace)
  bars: the captured K = 2 step -- the step a tracker runs in steady state -- is faster than D by more than the windows' spread
  ("v2_captured_minus_dense_us", "spread_dense_us", "bar_dense_met") at both M; V (K = 2, eager) is no slower than T beyond the
  spread ("v2_minus_stock_us", "bar_stock_met").  A missed bar ends the run with exit status 1 after the rows are written.
  Reported, not barred: "v2_eager_minus_dense_us" with "eager_faster_than_dense" (D allocates and runs eagerly only; the eager
  views step issues more launches than D and is bound by the host at small M) and "v2_over_single".
  G   nearest_views and gather_views alone (refs: V = 8 -> K = 2 rows of 8192 floats; the encoder's inputs: rows of 768 x 8 x 8),
      with the bytes they move and their share of the HBM peak (8 TB/s): they are expected to be launch-bound.

    python tools/bench_track_views.py [--out profiles/track_views_step.jsonl] [--only S,V,G] [--rounds 5] [--iters 200]
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_views_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_track_views.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    from tests import track_reference as tr
    from tests import track_views_reference as tvr
    P = tvr.TURN
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    W1, W2, b2 = (T(g[k]) for k in ("W1", "W2", "b2"))
    V, theta = P["views"], P["max_view_angle_deg"]
    X = T(tvr.turn_volume())
    A = T(tvr.turn_views())
    truth = tr.exp_so3(np.radians(10.0) * tvr.turn_axis()[None]).astype(np.float32)
    refs = ops.rotate_volume(X.expand(V, 16, 8, 8, 8), A)[None].contiguous()
    query = ops.rotate_volume(X, T(truth))
    R0 = T(rot.haar_rotations_np(P["n_init"], P["init_seed"]))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "V": V, "max_view_angle_deg": theta, "sigma_deg": P["sigma_deg"],
           "n_fresh": P["n_fresh"], "temperature": P["temperature"]}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    kw = dict(sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"], temperature=P["temperature"], batch=1, seed=0)

    def settle(t, *vols):
        t.init(*vols, R0)
        for _ in range(3):      # past the eager first step and both captures
            t.step(*vols)
        return t

    def dense_step(M):
        """Baseline 2: the tracker's chain with ops.verify_views over all V views as the scoring call."""
        t = ahv.track.PoseTracker(W1, W2, b2, particles=M, **kw)      # (borrowed for its buffers only)
        s0, k0 = ops.verify_views(refs, query, R0, A[None], W1, W2, b2, max_view_angle_deg=theta)
        state = {"R": R0, "s": s0, "key": k0, "p": 0, "ws": ops.resample_workspace(1, R0.shape[0], dev)}

        def f():
            p = state["p"]
            u = ops.track_advance(t._step, 0, 1, u=t._u)
            draws = ops.resample(state["s"], M, P["temperature"], u=u, out=t._draws, workspace=state["ws"])
            R = ops.diffuse_rotations(state["R"], idx=draws, sigma_deg=P["sigma_deg"], step=t._step, seed=0, best_key=state["key"],
                                      n_fresh=P["n_fresh"], out=t._R[p])
            s, key = ops.verify_views(refs, query, R, A[None], W1, W2, b2, max_view_angle_deg=theta, best_key=t._keys[p],
                                      reset_best=True)
            out = ops.select_rotation(key, R, out=t._sel[p])
            state.update(R=R, s=s, key=key, p=1 - p, ws=t._ws)
            return out
        return f

    def stock_glue_step(M, K):
        """Baseline 3: selection and gather in stock torch, then the tracker's own chain on the staged buffers."""
        t = settle(ahv.track.PoseTracker(W1, W2, b2, particles=M, views=A, views_per_step=K, max_view_angle_deg=theta, **kw),
                   refs, query)

        def f():
            tr_ = torch.einsum("bij,bvij->bv", t._anchor, t.views)
            idx = torch.argsort(tr_, dim=1, descending=True, stable=True)[:, :K]
            t._vsel.idx.copy_(idx)
            t._vsel.A.copy_(t.views[0].index_select(0, idx[0])[None])
            t.buffers[0].copy_(refs[0].index_select(0, idx[0])[None])
            t.buffers[1].copy_(query[:, None].expand(1, K, 16, 8, 8, 8))
            t._selected = True
            return t.step()
        return f

    missed = []
    if want("S") or want("V") or want("D") or want("T"):
        for M in (512, 2048):
            single = lambda **k: settle(ahv.track.PoseTracker(W1, W2, b2, particles=M, **kw, **k), refs[:, 0].contiguous(), query)
            views = lambda K, **k: settle(ahv.track.PoseTracker(W1, W2, b2, particles=M, views=A, views_per_step=K,
                                                                max_view_angle_deg=theta, **kw, **k), refs, query)
            se, sg = single(), single(use_graph=True)
            v2e, v2g, v8e, v8g = views(2), views(2, use_graph=True), views(8), views(8, use_graph=True)
            src0 = refs[:, 0].contiguous()
            sg.buffers[0].copy_(src0)
            sg.buffers[1].copy_(query)
            # (the captured steps replay on their static inputs: no staging copy, as in tools/bench_track.py)
            variants = {"S_single_eager": lambda: se.step(src0, query), "S_single_captured": lambda: sg.step(),
                        "V_k2_eager": lambda: v2e.step(refs, query), "V_k2_captured": lambda: v2g.step(*v2g.view_inputs),
                        "V_k8_eager": lambda: v8e.step(refs, query), "V_k8_captured": lambda: v8g.step(*v8g.view_inputs),
                        "D_dense_verify_views": dense_step(M), "T_k2_stock_torch_glue": stock_glue_step(M, 2),
                        "V_k2_eager_again": lambda: v2e.step(refs, query)}
            st = alternate(variants, a.rounds, a.iters)
            width = lambda k: st[k]["max_us"] - st[k]["min_us"]
            d_dense = st["V_k2_captured"]["us"] - st["D_dense_verify_views"]["us"]
            d_eager = st["V_k2_eager"]["us"] - st["D_dense_verify_views"]["us"]
            d_stock = st["V_k2_eager"]["us"] - st["T_k2_stock_torch_glue"]["us"]
            sp_dense = max(width("V_k2_captured"), width("D_dense_verify_views"))
            sp_eager = max(width("V_k2_eager"), width("D_dense_verify_views"))
            sp_stock = max(width("V_k2_eager"), width("T_k2_stock_torch_glue"))
            if not d_dense < -sp_dense:
                missed.append("M = %d: V(K=2, captured) - D = %.1f us, spread %.1f us" % (M, d_dense, sp_dense))
            if not d_stock <= sp_stock:
                missed.append("M = %d: V(K=2) - T = %.1f us, spread %.1f us" % (M, d_stock, sp_stock))
            for s in st.values():
                s.update(v2_captured_minus_dense_us=round(d_dense, 3), spread_dense_us=round(sp_dense, 3),
                         bar_dense_met=bool(d_dense < -sp_dense), v2_eager_minus_dense_us=round(d_eager, 3),
                         spread_eager_dense_us=round(sp_eager, 3), eager_faster_than_dense=bool(d_eager < -sp_eager),
                         v2_minus_stock_us=round(d_stock, 3), spread_stock_us=round(sp_stock, 3), bar_stock_met=bool(d_stock <= sp_stock),
                         v2_over_single=round(st["V_k2_eager"]["us"] / st["S_single_eager"]["us"], 3),
                         v2_captured_over_single_captured=round(st["V_k2_captured"]["us"] / st["S_single_captured"]["us"], 3))
            emit({"row": "SVDT", "B": 1, "M": M}, st)

    if want("G"):
        anchor = T(truth)
        sel = ops.nearest_views(anchor, A[None], 2)
        out_sel = ops.ViewSelection(sel.idx.clone(), sel.A.clone())
        out_refs = ops.gather_views(refs, sel.idx)
        l4 = torch.randn(1, V, 768, 8, 8, device=dev)
        out_l4 = ops.gather_views(l4, sel.idx)
        variants = {"G_nearest_views": lambda: ops.nearest_views(anchor, A[None], 2, out=out_sel),
                    "G_gather_volumes": lambda: ops.gather_views(refs, sel.idx, out=out_refs),
                    "G_gather_layer4": lambda: ops.gather_views(l4, sel.idx, out=out_l4)}
        moved = {"G_nearest_views": 4 * (9 + V * 9 + 2 + 2 * 9), "G_gather_volumes": 2 * 2 * 8192 * 4 + 8,
                 "G_gather_layer4": 2 * 2 * 768 * 64 * 4 + 8}      # read + written
        st = alternate(variants, a.rounds, a.iters)
        for k, s in st.items():
            s["bytes_moved"] = moved[k]
            s["share_of_hbm_peak"] = round(moved[k] / (s["us"] * 1e-6) / HBM_PEAK, 6)
        emit({"row": "G", "B": 1, "K": 2}, st)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if missed:
        sys.exit("bar missed: " + "; ".join(missed))


if __name__ == "__main__":
    main()
