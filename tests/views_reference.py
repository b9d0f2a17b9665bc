"""Numpy fp64 restatement of the multi-view fusion of ``ahv_view_rotations_f32`` / ``ahv_fuse_view_scores_f32`` (include/ahv.h,
"Multi-view verification").  Plain module (like tests/modes_reference.py).

Per sample: V reference views with absolute rotations A_v, N hypotheses Q_n of the query's absolute rotation, per-view scores
s_{v,n} of the relative rotation R_{v,n} = Q_n A_v^T.  View v PARTICIPATES in hypothesis n (g_{v,n} = 1) when w_v > 0 and
either no angle limit is given or t = sum_ab Q_n[a][b] A_v[a][b] >= tau, tau = 1 + 2 cos(theta_max) in double rounded to fp32;
a NaN t does not participate.  S_n = (sum_v g w_v s_{v,n}) / (sum_v g w_v) over v = 0 .. V-1, -inf when no view participates.
A view with w_v = 0 is absent (its scores never enter a sum, so 0 * NaN cannot occur); a participating NaN score makes S_n NaN.
The arg-max is the packed key (``dist.pack_keys_host``: signed int64 order = NaN above +inf, lowest index among equal scores,
-0 = +0) of (fp32 S_n, n_offset + n).

t is computed in fp64 here (the kernel: fp32), and the smallest |t - tau| over every decision is returned beside the result: a
test compares only where that margin is far above what fp32 rounding moves t by (~1e-6).
"""
import importlib
import math

import numpy as np

EMPTY = -(1 << 63)


def tau_of(max_view_angle_deg):
    return np.float32(1.0 + 2.0 * math.cos(math.radians(float(max_view_angle_deg))))


def view_rotations(Q, A):
    """Q (N,3,3) or (B,N,3,3), A (B,V,3,3) -> R (B,V,N,3,3) = Q_n A_v^T in fp64."""
    Q, A = np.asarray(Q, np.float64), np.asarray(A, np.float64)
    Qb = Q[None] if Q.ndim == 3 else Q
    return np.einsum("bnij,bvkj->bvnik", np.broadcast_to(Qb, (A.shape[0],) + Qb.shape[1:]), A)


def fuse(scores, Q, A, weights=None, max_view_angle_deg=None):
    """scores (B,V,N) fp32, Q (N,3,3) / (B,N,3,3), A (B,V,3,3), weights V floats or None ->
    ``(S (B,N) fp64, scale (B,N) = sum_v g w |s| / sum_v g w (NaN where it is not finite), g (B,V,N) bool, margin)``."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    B, V, N = s.shape
    w = np.ones(V, np.float32) if weights is None else np.asarray(weights, np.float32)
    assert w.shape == (V,) and np.all(np.isfinite(w)) and np.all(w >= 0) and np.any(w > 0)
    w = w.astype(np.float64)
    g = np.broadcast_to((w > 0)[None, :, None], (B, V, N)).copy()
    margin = np.inf
    if max_view_angle_deg is not None:
        tau = float(tau_of(max_view_angle_deg))
        Qd = np.asarray(Q, np.float64)
        Qb = np.broadcast_to(Qd[None] if Qd.ndim == 3 else Qd, (B, N, 3, 3))
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.einsum("bnij,bvij->bvn", Qb, np.asarray(A, np.float64))
            d = np.abs(t - tau)[:, w > 0]
            ok = ~np.isnan(d)
            if ok.any():
                margin = float(d[ok].min())
            g &= t >= tau                      # false for a NaN t
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S = np.zeros((B, N))
        scale = np.zeros((B, N))
        den = np.zeros((B, N))
        for v in range(V):                     # v = 0 .. V-1, in that order; an excluded term is never formed
            S = np.where(g[:, v], S + w[v] * s[:, v], S)
            scale = np.where(g[:, v], scale + w[v] * np.abs(s[:, v]), scale)
            den = np.where(g[:, v], den + w[v], den)
        S = np.where(den > 0, S / np.where(den > 0, den, 1.0), -np.inf)
        scale = np.where(den > 0, scale / np.where(den > 0, den, 1.0), np.nan)
    return S, scale, g, margin


def best_keys(S, n_offset=0):
    """(B,N) fused scores (rounded to fp32 here) -> (B,) packed arg-max keys: NaN first, lowest index among equal scores."""
    pack = importlib.import_module("3dahv_amd").dist.pack_keys_host
    with np.errstate(over="ignore"):
        s32 = np.asarray(S).astype(np.float32)
    B, N = s32.shape
    idx = np.broadcast_to(np.arange(N, dtype=np.int64) + n_offset, (B, N))
    return pack(s32, idx).reshape(B, N).max(axis=1)


def decode(keys):
    """(B,) keys -> (scores fp32, global indices)."""
    return importlib.import_module("3dahv_amd").dist.unpack_keys_host(np.asarray(keys))
