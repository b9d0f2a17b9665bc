"""What pose selection modulo a symmetry group costs (profiles/sym_step.jsonl).  The method is tools/bench_topk.py's: one process,
one GPU, profiler off, the variants timed ALTERNATELY (median of the rounds, min / max the spread), time-based warm-up.

One pair x 50 000 Haar hypotheses, theta = 15 degrees, K = 8 and 16, the octahedral group (G = 24) and C_inf:
  P   verify_pair_modes: the plain mode step (timed twice: P and P2 give the spread)
  S   verify_pair_modes(symmetry=): verify_pair(want_scores) + ahv_topk_modes_sym_f32 + select_topk; "ratio_to_P" = S / P
  D   the stock composition a user would write: verify_pair(want_scores), then K rounds of torch.max + the G traces against the
      winner by einsum (with an axis: the closed form) + masked_fill, then a gather
  F   ahv_sym_fold_f32 alone on 50 000 resident hypotheses, one anchor, no limit: time and the share of HBM bandwidth on the
      bytes it moves (72 B per hypothesis, + 12 for which / elem / trace, + 24 for V in and out)
  T   the tracker's step with and without symmetry at 512 and 2 048 particles, eager and captured

    python tools/bench_sym.py [--out profiles/sym_step.jsonl] [--only PSD,F,T] [--rounds 5] [--iters 200]
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

ANGLE = 15.0
HBM_GBS = 8000.0   # MI355X peak HBM3E bandwidth, GB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sym_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sym.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops, Sy = ahv.ops, ahv.rotations.Symmetry
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    gb = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    N = 50_000
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(N, 7)).to(dev)
    tau = ops.min_trace(ANGLE)
    groups = {"octahedral": Sy.octahedral().to(dev), "c_inf": Sy.axial((2.0, -1.0, 2.0)).to(dev)}
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "theta_deg": ANGLE}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

    def stock(k, sym):
        """Row D: the same selection with stock torch ops (its tie rule among equal scores is torch.max's)."""
        S, ax = sym.S, sym.axis

        def f():
            s, _ = ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True, best_key=key, reset_best=True)   # a fresh tensor
            idx = []
            for _ in range(k):
                _, i = torch.max(s, dim=1)
                idx.append(i)
                w = R[i[0]]
                if ax is None:
                    t = torch.einsum("nab,gbc,ac->ng", R, S, w).max(dim=1).values          # <R_n, R_w S_g^T>
                else:
                    M = torch.einsum("ba,nbc,gcd->ngad", w, R, S)                             # R_w^T R_n S_g
                    tr = M.diagonal(dim1=-2, dim2=-1).sum(-1)
                    p = torch.einsum("a,ngab,b->ng", ax, M, ax)
                    sn = -(ax[0] * (M[..., 2, 1] - M[..., 1, 2]) + ax[1] * (M[..., 0, 2] - M[..., 2, 0]) + ax[2] * (M[..., 1, 0] - M[..., 0, 1]))
                    t = (p + torch.sqrt((tr - p) ** 2 + sn ** 2)).max(dim=1).values
                s.masked_fill_((t >= tau)[None], -math.inf)
                s[0, i[0]] = -math.inf
            idx = torch.stack(idx, dim=1)
            return idx, R[idx]
        return f

    if want("PSD"):
        def step(k, sym):
            klist = torch.empty((1, k), dtype=torch.int64, device=dev)
            ws = ops.topk_modes_workspace(1, N, k, dev)
            return lambda: ops.verify_pair_modes(vs, vt, R, W1, W2, b2, k, ANGLE, keys=klist, workspace=ws, symmetry=sym,
                                                 best_key=key, reset_best=True)

        for k in (8, 16):
            variants = {"P_verify_pair_modes_K%d" % k: step(k, None), "P2_same_again_K%d" % k: step(k, None)}
            same = {}
            for name, sym in groups.items():
                variants["S_verify_pair_modes_sym_%s_K%d" % (name, k)] = step(k, sym)
                variants["D_verify_pair_torch_rounds_gather_%s_K%d" % (name, k)] = stock(k, sym)
                _, idx, _ = variants["S_verify_pair_modes_sym_%s_K%d" % (name, k)]()
                sidx, _ = variants["D_verify_pair_torch_rounds_gather_%s_K%d" % (name, k)]()
                same[name] = bool(torch.equal(idx, sidx))
            st = alternate(variants, a.rounds, a.iters)
            base = st["P_verify_pair_modes_K%d" % k]["us"]
            for name in groups:
                st["S_verify_pair_modes_sym_%s_K%d" % (name, k)]["same_list_as_D"] = same[name]
            for s in st.values():
                s["ratio_to_P"] = round(s["us"] / base, 3)
            emit({"row": "PSD", "B": 1, "N": N, "K": k}, st)

    if want("F"):
        Rb = R[None].contiguous()
        anchors = torch.from_numpy(ahv.rotations.haar_rotations_np(1, 3)).to(dev)[None]
        V = torch.randn(1, N, 3, device=dev) * 0.1
        out, vout = torch.empty_like(Rb), torch.empty_like(V)
        variants, moved = {}, {}
        for name, sym in groups.items():
            variants["F_sym_fold_%s" % name] = lambda sym=sym: ops.sym_fold(Rb, sym, anchors, None, out=out, want_info=False)
            moved["F_sym_fold_%s" % name] = 72
            variants["F_sym_fold_%s_info_V" % name] = lambda sym=sym: ops.sym_fold(Rb, sym, anchors, None, V=V, out=out, V_out=vout)
            moved["F_sym_fold_%s_info_V" % name] = 72 + 12 + 24
        st = alternate(variants, a.rounds, a.iters)
        for name, s in st.items():
            s["bytes_per_hypothesis"] = moved[name]
            s["hbm_share"] = round(moved[name] * N / (s["us"] * 1e-6) / (HBM_GBS * 1e9), 4)
        emit({"row": "F", "B": 1, "N": N, "K": 1}, st)

    if want("T"):
        vs1, vt1 = T(gb["vol_src"][:1]), T(gb["vol_tgt"][:1])
        sym = Sy.dihedral(2, "Z").to(dev)
        variants = {}
        for m in (512, 2048):
            for graph in (False, True):
                for label, s in (("plain", None), ("symmetry", sym)):
                    t = ahv.track.PoseTracker(W1, W2, b2, particles=m, n_fresh=m // 16, temperature=0.05, seed=1, use_graph=graph,
                                              symmetry=s)
                    t.init(vs1, vt1, R[:4096])
                    for _ in range(3):   # the eager step and the two capturing ones
                        t.step(vs1, vt1)
                    variants["T_track_step_M%d_%s_%s" % (m, "graph" if graph else "eager", label)] = \
                        (lambda t=t: t.step(vs1, vt1)) if not graph else (lambda t=t: t.step())
        emit({"row": "T", "B": 1}, alternate(variants, a.rounds, a.iters))

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
