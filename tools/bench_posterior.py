"""What the pose posterior costs (profiles/posterior_step.jsonl).  The method is tools/bench_modes.py's: one process, one GPU,
profiler off, the variants timed ALTERNATELY (median of the rounds, min / max the spread), time-based warm-up.

One pair x 50 000 hypotheses, theta = 15 degrees, T = 0.1, K = 8 and 16:
  A   verify_pair_modes: the step the posterior is added to
  B   verify_pair_posterior: A + ahv_pose_posterior_f32 + ahv_pose_posterior_finish_f32; "added_us_over_A" = B - A
  C   the stock composition on RESIDENT scores and anchors: torch.softmax, K masked sums with first-match assignment, einsum,
      torch.linalg.svd ("same_as_stock": B's numbers against C's within the tests' tolerances)
  M   ops.pose_posterior alone at N = 10 000 and 50 000 (state and workspace given)
The bar: B <= A + C, i.e. the kernel path adds no more than the stock composition costs.

    python tools/bench_posterior.py [--out profiles/posterior_step.jsonl] [--only ABC,M] [--rounds 5] [--iters 200]
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

ANGLE, TEMP = 15.0, 0.1


def stock_posterior(s, R, A, tau, beta):
    """Row C: what a user would write with stock torch ops.  s (1,N), R (N,3,3), A (1,K,3,3)."""
    K = A.shape[1]
    x = s * beta
    p = torch.softmax(x, dim=1)
    log_z = torch.logsumexp(x, dim=1)
    entropy = -(p * torch.log_softmax(x, dim=1)).sum(dim=1)
    mean_score = (p * s).sum(dim=1)
    left = torch.ones_like(s, dtype=torch.bool)
    masks = []
    for k in range(K):
        hit = left & (torch.einsum("nij,bij->bn", R, A[:, k]) >= tau) & (A[:, k] != 0).flatten(1).any(dim=1)[:, None]
        masks.append(hit)
        left = left & ~hit
    masks += [left, torch.ones_like(left)]
    W = torch.stack([p * m for m in masks], dim=1)
    mass = W.sum(dim=2)
    M = torch.einsum("bkn,nij->bkij", W, R)
    Mn = M / mass.clamp_min(1e-38)[..., None, None]
    U, _, Vt = torch.linalg.svd(Mn)
    d = torch.sign(torch.linalg.det(U @ Vt))
    Rm = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1)) @ Vt
    spread = torch.rad2deg(torch.acos((((Rm * Mn).sum(dim=(-2, -1)) - 1) / 2).clamp(-1, 1)))
    return log_z, entropy, mean_score, mass[:, :K], mass[:, K], Rm[:, :K], Rm[:, K + 1], spread[:, :K], spread[:, K + 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posterior_step.jsonl"))
    ap.add_argument("--only", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_posterior.py measures on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    ops = ahv.ops
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(REPO, "tests", "golden", "score_n128.npz"))
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vs, vt, W1, W2, b2 = (T(g[k]) for k in ("vol_src", "vol_tgt", "W1", "W2", "b2"))
    N = 50_000
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(N, 7)).to(dev)
    tau, beta = ops.min_trace(ANGLE), ops.inverse_temperature(TEMP)
    box = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "cu": ahv._lib.load().ahv_device_cu_count(), "theta_deg": ANGLE, "temperature": TEMP}
    rows = []

    def emit(row, stats):
        for name, st in stats.items():
            rows.append(dict(row, variant=name, **st, **box))
            print(json.dumps(rows[-1]), flush=True)

    want = lambda r: not a.only or r in a.only.split(",")
    key = torch.full((1,), ahv.dist.KEY_EMPTY, dtype=torch.int64, device=dev)

    if want("ABC"):
        variants, same = {}, {}
        for k in (8, 16):
            klist = torch.empty((1, k), dtype=torch.int64, device=dev)
            ws = ops.topk_modes_workspace(1, N, k, dev)
            variants["A_verify_pair_modes_K%d" % k] = (lambda k=k, kl=klist, ws=ws: ops.verify_pair_modes(
                vs, vt, R, W1, W2, b2, k, ANGLE, keys=kl, workspace=ws, best_key=key, reset_best=True))
            variants["B_verify_pair_posterior_K%d" % k] = (lambda k=k: ops.verify_pair_posterior(
                vs, vt, R, W1, W2, b2, k, ANGLE, temperature=TEMP, best_key=key, reset_best=True))
            scores = ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True, best_key=key, reset_best=True)[0]
            anchors = ops.select_topk(ops.topk_modes(scores, R, k, ANGLE), R)[2]
            variants["C_stock_posterior_on_resident_scores_K%d" % k] = (lambda s=scores, A=anchors: stock_posterior(s, R, A, tau, beta))
            post = variants["B_verify_pair_posterior_K%d" % k]()[3]
            ref = variants["C_stock_posterior_on_resident_scores_K%d" % k]()
            got = (post.log_z, post.entropy, post.mean_score, post.mode_prob, post.rest_prob, post.mode_R_mean, post.R_mean,
                   post.mode_spread_deg, post.spread_deg)
            tol = (2e-5, 2e-5, 2e-5, 2e-5, 2e-5, 4e-3, 4e-3, 0.16, 0.16)   # scalars; matrix entries (0.22 degrees); degrees
            same[k] = bool(all(torch.allclose(x, y, rtol=t, atol=t, equal_nan=True) for x, y, t in zip(got, ref, tol)))
        st = alternate(variants, a.rounds, a.iters)
        for k in (8, 16):
            A, B, C = (st[n % k]["us"] for n in ("A_verify_pair_modes_K%d", "B_verify_pair_posterior_K%d",
                                                   "C_stock_posterior_on_resident_scores_K%d"))
            st["B_verify_pair_posterior_K%d" % k].update(added_us_over_A=round(B - A, 3), same_as_stock=same[k],
                                                         bar_B_le_A_plus_C=bool(B <= A + C))
        emit({"row": "ABC", "B": 1, "N": N}, st)

    if want("M"):
        variants = {}
        for n in (10_000, 50_000):
            s = torch.rand(1, n, device=dev)
            Rn = R[:n].contiguous()
            for k in (8, 16):
                anchors = ops.select_topk(ops.topk_modes(s, Rn, k, ANGLE), Rn)[2]
                state, ws = ops.pose_posterior_state(1, k, dev), ops.pose_posterior_workspace(1, n, k, dev)
                variants["M_pose_posterior_N%d_K%d" % (n, k)] = (lambda s=s, Rn=Rn, A=anchors, st=state, ws=ws: ops.pose_posterior(
                    s, Rn, TEMP, anchors=A, min_angle_deg=ANGLE, state=st, workspace=ws, reset=True))
        emit({"row": "M", "B": 1}, alternate(variants, a.rounds, a.iters))

    torch.cuda.synchronize()
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
