"""What joint pose inference over an unposed image set costs (profiles/pose_graph_step.jsonl).  The method is
tools/bench_track_cv.py's: one process, one GPU, profiler off, the variants timed ALTERNATELY (median of the windows, min / max
the spread), time-based warm-up.

V = 8 images, the complete ordered graph (E = 56 edges, every node of degree 14), one sample, N0 = 50 000 shared Haar hypotheses
for the pairwise stage, N = 512 candidates per node update, 8 sweeps (sigma = 6, 4, 3, 2, 1.5, 1, 0.75, 0.5 degrees); the
volumes are the planted graph of tests/pose_graph_reference.py with 5 bad edges:
  P   the pairwise stage alone (verify_pair over the 56 samples and select_rotation), the tree launch alone, one node update
      (pose_graph_propose -> pose_graph_score -> pose_graph_commit) and its three parts
  S   everything after the pairwise stage (PoseGraph.ascend: counter, tree, staging, 8 sweeps x 7 nodes), eager and captured,
      against the same ascent with the graph-level glue in stock torch around the SAME scoring launch: einsum for both rotation
      forms and the neighbours' proposals, torch.randn noise through the matrix exponential, mean, argmax, indexing.  The
      stock ascent is timed eagerly with torch.linalg.matrix_exp and, eagerly and captured, with the closed form of that
      exponential on so(3) (Rodrigues, sin / cos / matmul: torch.linalg.matrix_exp reads norms on the host and cannot be
      captured).  "kernels_minus_stock_us" and "spread_us" (the larger window spread of the two) per mode; the expectation --
      the kernel path is at or below the stock composition by more than the spread -- is reported, met or not.
  Q   the planted graph of the tests on the device (V = 5, 3 bad edges, seeds 0, 1, 2; N0 = 4 096, N = 256, 8 sweeps): joint
      max / median over all ordered pairs, the tree's max, pairwise clean median / max, the bad edges' pairwise errors

    python tools/bench_pose_graph.py [--out profiles/pose_graph_step.jsonl] [--only P,S] [--rounds 5] [--iters 200]
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

V, N0, N, SWEEPS, N_BAD = 8, 50_000, 512, 8, 5
VOL = (16, 8, 8, 8)


def skew(w):
    K = torch.zeros(w.shape[:-1] + (3, 3), dtype=w.dtype, device=w.device)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return K


def rodrigues(w):
    a = w.norm(dim=-1, keepdim=True).clamp_min(1e-12)[..., None]
    K = skew(w)
    return torch.eye(3, device=w.device) + (torch.sin(a) / a) * K + ((1 - torch.cos(a)) / (a * a)) * (K @ K)


class StockAscent:
    """The ascent of posegraph.PoseGraph with every graph-level step in stock torch; the scoring launch is ops.verify_pair's."""

    def __init__(self, ahv, graph, head, exp):
        self.ops, self.g, self.head, self.exp = ahv.ops, graph, head, exp
        dev = head[0].device
        top = graph.topology
        self.A = torch.eye(3, device=dev).repeat(1, V, 1, 1)
        self.node_score = torch.zeros((1, V), device=dev)
        self.scores = {k: torch.empty((top.degree[k], N), device=dev) for k in graph.nodes}
        self.keys = {k: torch.empty((top.degree[k],), dtype=torch.int64, device=dev) for k in graph.nodes}
        ix = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.plan = {}
        for k in graph.nodes:
            inc = top.incident[k]
            self.plan[k] = (ix([e for e, _ in inc]), ix([top.edges[e][1] if out else top.edges[e][0] for e, out in inc]),
                            torch.tensor([out for _, out in inc], device=dev)[None, :, None, None])
        self.zero = ix([0])

    def run(self, init_A, pair_R):
        g, ops = self.g, self.ops
        self.A.copy_(init_A)
        for s in range(SWEEPS):
            sigma = math.radians(g.sigma_deg[min(s, len(g.sigma_deg) - 1)])
            for k in g.nodes:
                e, other, out = self.plan[k]
                D = e.numel()
                cur, nb, P = self.A[:, k], self.A[:, other], pair_R[:, e]                       # (1,3,3), (1,D,3,3), (1,D,3,3)
                w = torch.randn((1, N, 3), device=cur.device) * sigma
                Q = cur[:, None] @ self.exp(w if self.exp is rodrigues else skew(w))
                Q[:, 0] = cur
                Q[:, 1:1 + D] = torch.where(out, torch.einsum("bdji,bdjk->bdik", P, nb), torch.einsum("bdij,bdjk->bdik", P, nb))
                Rrel = torch.where(out[..., None], torch.einsum("bdij,bnkj->bdnik", nb, Q), torch.einsum("bnij,bdkj->bdnik", Q, nb))
                ops.verify_pair(g._staged[k][0][0], g._staged[k][1][0], Rrel[0].contiguous(), *self.head, best_key=self.keys[k],
                                reset_best=True, scores_out=self.scores[k])
                fused = self.scores[k].mean(dim=0)
                idx = fused.argmax()
                self.A[0, k] = Q[0].index_select(0, idx[None])[0]
                self.node_score[0, k] = fused.index_select(0, idx[None])[0]
        return self.A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_graph_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pose_graph.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, rot = ahv.ops, ahv.rotations
    from tests import pose_graph_reference as pgr
    dev = torch.device("cuda:0")
    g128 = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    head = tuple(T(g128[k]) for k in ("W1", "W2", "b2"))
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count()}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    rotate = lambda vol, R: ops.rotate_volume(T(vol), T(np.asarray(R, np.float32)[None])).cpu().numpy()
    shape = {"V": V, "E": V * (V - 1), "D": 2 * (V - 1), "B": 1, "N0": N0, "N": N, "sweeps": SWEEPS, "bad_edges": N_BAD}

    if want("P") or want("S"):
        vs, vt, truth, bad = pgr.planted_volumes(rotate, rot, V, N_BAD, 0)
        vs, vt = T(vs), T(vt)
        R0 = ops.random_rotations(N0, seed=100, device=dev)
        make = lambda graph: ahv.posegraph.PoseGraph(*head, n_views=V, candidates=N, sweeps=SWEEPS, sigma_deg=pgr.SIGMA_DEG, seed=0,
                                                     use_graph=graph)
        eager, captured = make(False), make(True)
        res = eager.solve(vs, vt, R0)
        captured.solve(vs, vt, R0)
        fig = pgr.planted_figures(res.A[0].cpu().numpy(), res.pair_R[0].cpu().numpy(), res.parent_edge[0].cpu().numpy(), truth, bad, V)
        shape["joint_max_deg"], shape["pair_clean_median_deg"] = round(fig["joint_max"], 3), round(fig["pair_clean_median"], 3)
        E = eager.E
    if want("P"):
        top, k = eager.topology, 1
        key, sel = torch.empty((E,), dtype=torch.int64, device=dev), eager._pair
        A, ns = res.A.clone(), res.node_score.clone()
        Q, Rrel = eager._Q, eager._Rrel[k]
        propose = lambda: ops.pose_graph_propose(A, res.pair_R, res.pair_score, top, k, N, 1.0, sweep=3, counter=eager.counter, out=(Q, Rrel))
        score = lambda: ops.pose_graph_score(eager._staged[k][0], eager._staged[k][1], Rrel, *head, workspace=eager._ws[k],
                                             scores_out=eager._fused, best_key=eager._key)
        commit = lambda: ops.pose_graph_commit(eager._key, Q, A, ns, k)
        propose(), score()
        st = alternate({
            "pairwise_stage": lambda: (ops.verify_pair(vs.view((E,) + VOL), vt.view((E,) + VOL), R0, *head, want_scores=False, best_key=key,
                                                       reset_best=True), ops.select_rotation(key, R0, out=sel)),
            "tree_launch": lambda: ops.pose_graph_init(res.pair_R, res.pair_score, top, out=(A, res.parent_edge, res.reached)),
            "node_update": lambda: (propose(), score(), commit()),
            "propose": propose, "score_and_fuse": score, "commit": commit,
        }, a.rounds, a.iters)
        emit(dict(shape, row="P"), st)
    if want("S"):
        stock_exp, stock_rod = (StockAscent(ahv, eager, head, e) for e in (torch.linalg.matrix_exp, rodrigues))
        init_A, pair_R = res.init_A.clone(), res.pair_R.clone()
        stock_rod.run(init_A, pair_R)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            stock_rod.run(init_A, pair_R)
        graph.replay()
        torch.cuda.synchronize()
        fig_s = pgr.planted_figures(stock_rod.A[0].cpu().numpy(), res.pair_R[0].cpu().numpy(), res.parent_edge[0].cpu().numpy(), truth, bad, V)
        st = alternate({
            "kernels_eager": eager.ascend, "kernels_captured": captured.ascend,
            "stock_eager_matrix_exp": lambda: stock_exp.run(init_A, pair_R), "stock_eager_rodrigues": lambda: stock_rod.run(init_A, pair_R),
            "stock_captured_rodrigues": graph.replay,
        }, a.rounds, max(a.iters // 10, 5))
        for ours, theirs in (("kernels_eager", "stock_eager_matrix_exp"), ("kernels_eager", "stock_eager_rodrigues"),
                             ("kernels_captured", "stock_captured_rodrigues")):
            o, t = st[ours], st[theirs]
            spread = max(o["max_us"] - o["min_us"], t["max_us"] - t["min_us"])
            t.update(kernels_minus_stock_us=round(o["us"] - t["us"], 3), spread_us=round(spread, 3),
                     kernels_faster_by_more_than_spread=bool(t["us"] - o["us"] > spread))
        emit(dict(shape, row="S", stock_joint_max_deg=round(fig_s["joint_max"], 3)), st)

    if want("Q"):
        for seed in (0, 1, 2):
            v, n_bad = 5, 3
            vs5, vt5, truth, bad = pgr.planted_volumes(rotate, rot, v, n_bad, seed)
            g = ahv.posegraph.PoseGraph(*head, n_views=v, candidates=256, sweeps=8, sigma_deg=pgr.SIGMA_DEG, seed=seed)
            r = g.solve(T(vs5), T(vt5), ops.random_rotations(4096, seed=100 + seed, device=dev))
            host = lambda t: t[0].cpu().numpy()
            fig = pgr.planted_figures(host(r.A), host(r.pair_R), host(r.parent_edge), truth, bad, v)
            tree = pgr.planted_figures(host(r.init_A), host(r.pair_R), host(r.parent_edge), truth, bad, v)
            rows.append(dict({"row": "Q", "V": v, "bad_edges": bad, "seed": seed, "N0": 4096, "N": 256, "sweeps": 8,
                              "tree_max_deg": round(tree["joint_max"], 3)},
                             **{k: ([round(x, 1) for x in val] if isinstance(val, list) else round(val, 3)) for k, val in fig.items()}, **box))
            print(json.dumps(rows[-1]), flush=True)

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
