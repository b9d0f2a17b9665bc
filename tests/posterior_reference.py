"""Numpy restatement of the pose posterior of ``ahv_pose_posterior_f32`` / ``_merge`` / ``_finish_f32`` (include/ahv.h, "Pose
posterior"), in fp64 from the fp32 inputs.  Plain module (like tests/modes_reference.py).

A STATE of one sample is a dict ``{"n_excluded": int, "rec": (K + 2, 12) float64}``: records of buckets 0 .. K-1, the rest
bucket and the whole set, each ``[m, mass, S, M (9)]`` relative to its own m (``[-inf, 0, ...]`` when empty) -- the layout the
header documents, so ``to_bytes`` / ``from_bytes`` convert to and from what the library reads and writes.  Beside the results
``posterior`` returns the smallest |t - min_trace| over every assignment decision made and, per bucket, the conditioning
sigma_2 + sigma_3 of M / mass: a test compares bucket contents only where the margin is far above what an fp32 summation order
can move t by (~1e-6), and mean rotations only where the projection is well conditioned.
"""
import math

import numpy as np

REC = 12
HEADER = 16


def beta_of(temperature):
    """beta = 1 / T: double precision, rounded to fp32 (what the host passes to the kernels)."""
    return np.float32(1.0 / float(temperature))


def tau_of(min_angle_deg):
    return np.float32(1.0 + 2.0 * math.cos(math.radians(float(min_angle_deg))))


def state_stride(K):
    return HEADER + (K + 2) * REC * 8


def haar(rng, n):
    """n Haar-uniform rotations (n,3,3) fp32 from a numpy Generator (normalised Gaussian quaternions)."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(n, 3, 3).astype(np.float32)


def geodesic_deg(A, B):
    """Geodesic angle in degrees between rotations (...,3,3), the metric of test_co3d.py:149-150."""
    t = np.sum(np.asarray(A, np.float64) * np.asarray(B, np.float64), axis=(-2, -1))
    return np.degrees(np.arccos(np.clip((t - 1.0) / 2.0, -1.0, 1.0)))


def planted_scores(R, peaks, heights=(0.9, 0.8), width_deg=40.0):
    """s_i = max_k h_k exp(-(angle(R_i, P_k) / width)^2), fp32."""
    s = np.max([h * np.exp(-(geodesic_deg(R, P[None]) / width_deg) ** 2) for h, P in zip(heights, peaks)], axis=0)
    return s.astype(np.float32)


def make_inputs(N, B, per_sample, seed, K=4, angle_deg=30.0):
    """The GPU tests' inputs: Haar rotations (shared (N,3,3) or per sample (B,N,3,3)), planted-peak scores (B,N) around two
    random poses per sample, and as anchors (B,K,3,3) the rotations of ``modes_reference.select_modes`` at ``angle_deg`` (zero
    matrices past the last mode)."""
    from . import modes_reference as mr
    rng = np.random.default_rng(seed)
    R = haar(rng, N * B).reshape(B, N, 3, 3) if per_sample else haar(rng, N)
    peaks = haar(rng, 2 * B).reshape(B, 2, 3, 3)
    s = np.stack([planted_scores(R[b] if per_sample else R, peaks[b]) for b in range(B)])
    anchors = np.zeros((B, K, 3, 3), np.float32)
    if K:
        idx = mr.indices(mr.select_modes(s, R, K, angle_deg)[0])
        for b in range(B):
            for k in range(K):
                if idx[b, k] >= 0:
                    anchors[b, k] = (R[b] if per_sample else R)[idx[b, k]]
    return s, R, anchors


def empty_state(K):
    rec = np.zeros((K + 2, REC), np.float64)
    rec[:, 0] = -np.inf
    return {"n_excluded": 0, "rec": rec}


def assign(R, anchors, tau):
    """Bucket of every hypothesis (first matching non-empty anchor, else K) and the smallest |t - tau| met.  R (N,3,3),
    anchors (K,3,3)."""
    N, K = len(R), len(anchors)
    bucket = np.full(N, K, dtype=np.int64)
    margin = np.inf
    Rf = np.asarray(R, np.float64).reshape(N, 9)
    for k in range(K - 1, -1, -1):
        A = np.asarray(anchors[k], np.float64).reshape(9)
        if not np.any(np.asarray(anchors[k]) != 0):   # an empty slot: skipped by its flag, not by its value
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            t = Rf @ A
            d = np.abs(t - float(tau))
            hit = t >= float(tau)                      # false for a NaN t
        ok = ~np.isnan(d)
        if ok.any():
            margin = min(margin, float(d[ok].min()))
        bucket[hit] = k
    return bucket, margin


def state_of(scores, R, anchors, tau, beta):
    """One sample: scores (N,), R (N,3,3), anchors (K,3,3) -> (state, margin)."""
    s32 = np.asarray(scores, np.float32)
    N, K = len(s32), len(anchors)
    st = empty_state(K)
    fin = np.isfinite(s32)
    st["n_excluded"] = int(N - fin.sum())
    bucket, margin = assign(R, anchors, tau) if N else (np.zeros(0, np.int64), np.inf)
    s = s32.astype(np.float64)
    Rf = np.asarray(R, np.float64).reshape(N, 9)
    for j in range(K + 2):
        sel = fin if j == K + 1 else fin & (bucket == j)
        if not sel.any():
            continue
        m = s[sel].max()
        w = np.exp((s[sel] - m) * float(beta))
        st["rec"][j, 0], st["rec"][j, 1], st["rec"][j, 2] = m, w.sum(), (w * s[sel]).sum()
        st["rec"][j, 3:] = (w[:, None] * Rf[sel]).sum(axis=0)
    return st, margin


def merge(a, b, beta):
    """The online-softmax merge rule, record by record: m = max, each side rescaled by exp((m_side - m) beta)."""
    out = {"n_excluded": a["n_excluded"] + b["n_excluded"], "rec": a["rec"].copy()}
    for j in range(len(out["rec"])):
        ma, mb = a["rec"][j, 0], b["rec"][j, 0]
        m = max(ma, mb)
        if m == -np.inf:
            continue
        fa = 0.0 if ma == -np.inf else math.exp((ma - m) * float(beta))
        fb = 0.0 if mb == -np.inf else math.exp((mb - m) * float(beta))
        out["rec"][j, 1:] = a["rec"][j, 1:] * fa + b["rec"][j, 1:] * fb
        out["rec"][j, 0] = m
    return out


def nearest_rotation(M):
    """U diag(1, 1, det(U V^T)) V^T and the singular values of M (3,3)."""
    U, sv, Vt = np.linalg.svd(M)
    d = np.sign(np.linalg.det(U @ Vt))
    return U @ np.diag([1.0, 1.0, d]) @ Vt, sv


def finish(st, beta):
    """A state -> dict of the outputs of one sample (fp64) plus ``cond`` (K + 2,): sigma_2 + sigma_3 of M / mass per record
    (NaN for an empty one; index K is the rest bucket, K + 1 the whole set)."""
    rec = st["rec"]
    K = len(rec) - 2
    beta = float(beta)
    m, Z, S = rec[K + 1, 0], rec[K + 1, 1], rec[K + 1, 2]
    out = {"n_excluded": st["n_excluded"]}
    if Z > 0:
        out["log_z"] = m * beta + math.log(Z)
        out["entropy"] = math.log(Z) - beta * (S / Z - m)
        out["mean_score"] = S / Z
    else:
        out["log_z"], out["entropy"], out["mean_score"] = -np.inf, np.nan, np.nan
    prob = np.zeros(K + 2)
    Rm = np.zeros((K + 2, 3, 3))
    spread = np.full(K + 2, np.nan)
    cond = np.full(K + 2, np.nan)
    for j in range(K + 2):
        if not rec[j, 1] > 0:
            continue
        prob[j] = rec[j, 1] * math.exp((rec[j, 0] - m) * beta) / Z
        M = rec[j, 3:].reshape(3, 3) / rec[j, 1]
        Rm[j], sv = nearest_rotation(M)
        cond[j] = sv[1] + sv[2]
        spread[j] = np.degrees(np.arccos(np.clip((np.sum(Rm[j] * M) - 1.0) / 2.0, -1.0, 1.0)))
    out.update(mode_prob=prob[:K], rest_prob=prob[K], mode_R_mean=Rm[:K], R_mean=Rm[K + 1], mode_spread_deg=spread[:K],
               spread_deg=spread[K + 1], cond=cond)
    return out


FIELDS = ("log_z", "entropy", "mean_score", "n_excluded", "mode_prob", "rest_prob", "mode_R_mean", "R_mean", "mode_spread_deg",
          "spread_deg")


def stack(outs):
    """Per-sample output dicts -> one dict of arrays with the batch in front."""
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def batch_states(scores, R, anchors, min_angle_deg, temperature):
    """scores (B,N) fp32, R (N,3,3) or (B,N,3,3), anchors (B,K,3,3) or None -> (list of B states, margin)."""
    scores = np.asarray(scores, np.float32)
    B = scores.shape[0]
    anchors = np.zeros((B, 0, 3, 3), np.float32) if anchors is None else np.asarray(anchors, np.float32)
    tau = tau_of(min_angle_deg) if anchors.shape[1] else np.float32(0.0)
    beta = beta_of(temperature)
    states, margin = [], np.inf
    for b in range(B):
        st, mg = state_of(scores[b], R[b] if np.ndim(R) == 4 else R, anchors[b], tau, beta)
        states.append(st)
        margin = min(margin, mg)
    return states, margin


def posterior(scores, R, anchors=None, min_angle_deg=None, temperature=0.1):
    """-> (dict of batched outputs incl. ``cond`` (B, K + 2), margin)."""
    states, margin = batch_states(scores, R, anchors, min_angle_deg, temperature)
    return stack([finish(st, beta_of(temperature)) for st in states]), margin


def to_bytes(states):
    """List of B states -> (B, stride) uint8, the library's layout."""
    K = len(states[0]["rec"]) - 2
    buf = np.zeros((len(states), state_stride(K)), np.uint8)
    for b, st in enumerate(states):
        buf[b, :HEADER].view(np.int64)[:] = (st["n_excluded"], 0)
        buf[b, HEADER:].view(np.float64)[:] = st["rec"].reshape(-1)
    return buf


def from_bytes(buf, K):
    """(B, stride) uint8 -> list of B states."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1, state_stride(K))
    return [{"n_excluded": int(row[:HEADER].view(np.int64)[0]), "rec": row[HEADER:].view(np.float64).reshape(K + 2, REC).copy()}
            for row in buf]


def stock_fp32(scores, R, anchors=None, min_angle_deg=None, temperature=0.1):
    """The stock fp32 torch composition on the CPU (softmax, K masked sums with first-match assignment, einsum,
    torch.linalg.svd): what a user would write without the kernels, and the yardstick of the kernels' tolerance.  Finite
    scores only (it has no notion of an excluded hypothesis).  Returns the same dict as ``posterior`` minus ``cond``."""
    import torch
    s = torch.from_numpy(np.asarray(scores, np.float32))
    B, N = s.shape
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float32))
    Rb = Rt if Rt.dim() == 4 else Rt[None].expand(B, N, 3, 3)
    A = torch.zeros((B, 0, 3, 3)) if anchors is None else torch.from_numpy(np.asarray(anchors, np.float32))
    K = A.shape[1]
    beta = float(beta_of(temperature))
    x = s * beta
    p = torch.softmax(x, dim=1)
    log_z = torch.logsumexp(x, dim=1)
    entropy = -(p * torch.log_softmax(x, dim=1)).sum(dim=1)
    mean_score = (p * s).sum(dim=1)
    left = torch.ones((B, N), dtype=torch.bool)
    masks = []
    for k in range(K):
        used = (A[:, k] != 0).flatten(1).any(dim=1)
        t = torch.einsum("bnij,bij->bn", Rb, A[:, k])
        hit = left & (t >= float(tau_of(min_angle_deg))) & used[:, None]
        masks.append(hit)
        left = left & ~hit
    masks += [left, torch.ones((B, N), dtype=torch.bool)]
    W = torch.stack([p * mk for mk in masks], dim=1)                  # (B, K + 2, N)
    mass = W.sum(dim=2)
    M = torch.einsum("bkn,bnij->bkij", W, Rb)
    Mn = M / mass.clamp_min(1e-38)[..., None, None]
    U, _, Vt = torch.linalg.svd(Mn)
    d = torch.sign(torch.linalg.det(U @ Vt))
    Rm = U @ torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1)) @ Vt
    spread = torch.rad2deg(torch.acos((((Rm * Mn).sum(dim=(-2, -1)) - 1) / 2).clamp(-1, 1)))
    none = mass <= 0
    Rm[none] = 0
    spread[none] = float("nan")
    n = lambda t: t.numpy().astype(np.float64)
    return {"log_z": n(log_z), "entropy": n(entropy), "mean_score": n(mean_score), "n_excluded": np.zeros(B, np.int64),
            "mode_prob": n(mass[:, :K]), "rest_prob": n(mass[:, K]), "mode_R_mean": n(Rm[:, :K]), "R_mean": n(Rm[:, K + 1]),
            "mode_spread_deg": n(spread[:, :K]), "spread_deg": n(spread[:, K + 1])}


def errors(got, want, cond=None, min_cond=0.5):
    """Largest error per class between two output dicts: ``scalar`` (log_z, entropy, mean_score, probabilities: absolute, or
    relative above 1e-2 in magnitude), ``rot_deg`` (geodesic angle of the mean rotations, only for buckets whose ``cond`` is
    at least ``min_cond``), ``spread_deg``."""
    def sc(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin], equal_nan=True), "non-finite values differ"
        d = np.abs(a[fin] - b[fin])
        return float(np.max(np.where(np.abs(b[fin]) > 1e-2, d / np.maximum(np.abs(b[fin]), 1e-2), d), initial=0.0))
    scalar = max(sc(got[k], want[k]) for k in ("log_z", "entropy", "mean_score", "mode_prob", "rest_prob"))
    K = np.asarray(want["mode_prob"]).shape[1]
    Rg = np.concatenate([np.asarray(got["mode_R_mean"], np.float64), np.asarray(got["R_mean"], np.float64)[:, None]], axis=1)
    Rw = np.concatenate([np.asarray(want["mode_R_mean"], np.float64), np.asarray(want["R_mean"], np.float64)[:, None]], axis=1)
    sg = np.concatenate([np.asarray(got["mode_spread_deg"], np.float64), np.asarray(got["spread_deg"], np.float64)[:, None]], axis=1)
    sw = np.concatenate([np.asarray(want["mode_spread_deg"], np.float64), np.asarray(want["spread_deg"], np.float64)[:, None]], axis=1)
    live = ~np.isnan(sw)
    assert np.array_equal(np.isnan(sg), ~live), "empty buckets differ"
    assert np.all(Rg[~live] == 0) and np.all(Rw[~live] == 0)
    ok = live if cond is None else live & (np.asarray(cond)[:, list(range(K)) + [K + 1]] >= min_cond)
    rot = float(np.max(geodesic_deg(Rg[ok], Rw[ok]), initial=0.0))
    spr = float(np.max(np.abs(sg[live] - sw[live]), initial=0.0))
    return {"scalar": scalar, "rot_deg": rot, "spread_deg": spr}
