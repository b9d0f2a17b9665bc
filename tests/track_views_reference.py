"""numpy restatement of the view selection and staging of ``ahv_nearest_views_f32`` / ``ahv_gather_views_f32`` (include/ahv.h), the
full-turn plant both test tiers track, and the oracle-backed CPU backend of ``track.PoseTracker(views=...)``.  Plain module.

    trace32        t = sum_ab anchor[a][b] A_v[a][b] as ONE fp32 fma chain over the nine entries in memory order, exactly:
                   a product of two floats is exact in a double, the sum is rounded to odd there (TwoSum gives the error) and
                   then once to float -- a correctly rounded fp32 fma.
    nearest_views  the K first views in the order: t descending, equal t by the lower v, a NaN t behind every number and NaNs
                   among themselves by v.
"""
import math

import numpy as np

from . import track_reference as tr
from . import views_reference as vr


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, for scalars."""
    a, b, c = np.float64(np.float32(a)), np.float64(np.float32(b)), np.float64(np.float32(c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                  # exact: 24 + 24 bits
        s = p + c
        if not np.isfinite(s):
            return np.float32(s)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)            # TwoSum: s + err = p + c exactly
        if err != 0.0 and not (s.view(np.int64) & 1):
            s = np.nextafter(s, np.float64(np.inf) if err > 0 else np.float64(-np.inf))   # round to odd
        return np.float32(s)


def trace32(anchor, A):
    """anchor (3,3), A (3,3) fp32 -> the fp32 t of the kernels' chain."""
    q, a = np.asarray(anchor, np.float32).reshape(9), np.asarray(A, np.float32).reshape(9)
    acc = np.float32(0.0)
    for i in range(9):
        acc = fma32(q[i], a[i], acc)
    return acc


def traces(anchor, A):
    """anchor (B,3,3), A (B,V,3,3) -> t (B,V) fp32."""
    B, V = np.asarray(A).shape[:2]
    return np.array([[trace32(anchor[b], A[b][v]) for v in range(V)] for b in range(B)], np.float32)


def order(t):
    """t (V,) fp32 -> the views in selection order."""
    nan = np.isnan(t)
    return sorted(range(len(t)), key=lambda v: (bool(nan[v]), 0.0 if nan[v] else -float(t[v]), v))


def nearest_views(anchor, A, k):
    """-> (idx (B,k) int32, A_sel (B,k,3,3): the rows of A, their bits)."""
    A = np.asarray(A, np.float32)
    t = traces(np.asarray(anchor, np.float32), A)
    idx = np.array([order(t[b])[:k] for b in range(len(A))], np.int32)
    return idx, A[np.arange(len(A))[:, None], idx]


def gather_views(src, idx, broadcast=False):
    """src (B,V,...) or, broadcast, (B,...); idx (B,K) -> (B,K,...); an index outside 0..V-1 gives zeros."""
    src, idx = np.asarray(src), np.asarray(idx)
    B, K = idx.shape
    if broadcast:
        return np.repeat(src[:, None], K, axis=1)
    V = src.shape[1]
    ok = (idx >= 0) & (idx < V)
    out = src[np.arange(B)[:, None], np.where(ok, idx, 0)].copy()
    out[~ok] = 0
    return out


# ---- the full turn ------------------------------------------------------------------------------------------------------
# One object volume X, V = 8 reference views A_v = exp(45 v [a]x) with refs_v = rotate_volume(X, A_v), the truth Q_t =
# exp(3 t [a]x) over 120 frames with query_t = rotate_volume(X, Q_t): every pose on the one axis, where Q commutes with every
# A_v and the plant is consistent under the Q A_v^T convention; the maximum of every view's score is at the truth.
TURN = dict(frames=120, deg_per_frame=3.0, views=8, view_step_deg=45.0, views_per_step=2, max_view_angle_deg=60.0, particles=512,
            sigma_deg=3.0, n_fresh=32, temperature=0.02, n_init=4096, init_seed=1000, axis=(0.48, -0.6, 0.64), volume_seed=17,
            late=6, blind_every=12)


def turn_axis():
    a = np.asarray(TURN["axis"], np.float64)
    return a / np.linalg.norm(a)


def turn_volume():
    return np.random.default_rng(TURN["volume_seed"]).standard_normal((1, 16, 8, 8, 8)).astype(np.float32)


def turn_views():
    """(V,3,3) fp32."""
    v = np.arange(TURN["views"], dtype=np.float64)[:, None]
    return tr.exp_so3(v * math.radians(TURN["view_step_deg"]) * turn_axis()[None]).astype(np.float32)


def turn_truth(frames=None):
    """(frames,3,3) fp64."""
    t = np.arange(TURN["frames"] if frames is None else frames, dtype=np.float64)[:, None]
    return tr.exp_so3(t * math.radians(TURN["deg_per_frame"]) * turn_axis()[None])


def turn_bar(track_err, blind_err):
    """The bar: the tracker's largest error from frame 6 on stays below the median error of the blind fused arg-max on every
    12th frame.  ``blind_err`` holds only those frames.  Returns (tracker max, blind median)."""
    return float(np.max(np.asarray(track_err)[TURN["late"]:])), float(np.median(np.asarray(blind_err)))


# ---- oracle-backed CPU backend of track.PoseTracker(views=...) -----------------------------------------------------------
def make_backend(ahv, oracle):
    """``track_reference.make_backend`` plus ``nearest_views``, ``gather_views`` and ``verify_views_staged``: the selection and
    the gather are this module's, the scores the CPU oracle's per (view, query) sample, the fusion ``views_reference.fuse``
    rounded to fp32.  Test infrastructure: the product backend is HIP."""
    import torch

    base = tr.make_backend(ahv, oracle)

    class TrackViewsOracleBackend(type(base)):
        def nearest_views(self, anchor, A, k, out=None):
            idx, A_sel = nearest_views(anchor.numpy(), A.numpy(), k)
            res = ahv.ops.ViewSelection(torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(A_sel)))
            if out is not None:
                out.idx.copy_(res.idx)
                out.A.copy_(res.A)
                res = out
            self.calls.append("nearest_views")
            return res

        def gather_views(self, src, idx, out=None, broadcast=False):
            res = torch.from_numpy(np.ascontiguousarray(gather_views(src.numpy(), idx.numpy(), broadcast)))
            if out is not None:
                out.copy_(res)
                res = out
            self.calls.append("gather_views")
            return res

        def verify_views_staged(self, vol_refs, vol_query, Q, A_sel, W1, W2, b2, max_view_angle_deg=None, workspace=None,
                                scores_out=None, best_key=None, reset_best=None, split_f16=None):
            B, K = A_sel.shape[:2]
            Qn, An = Q.numpy(), A_sel.numpy()
            Rv = vr.view_rotations(Qn, An).astype(np.float32)                     # (B,K,N,3,3)
            N = Rv.shape[2]
            vq = vol_query.numpy()
            if vq.ndim == 5:
                vq = np.repeat(vq[:, None], K, axis=1)
            refs = vol_refs.numpy()
            w = (W1.numpy(), W2.numpy(), b2.numpy())
            # a pair outside the angle never enters a sum (views_reference.fuse): only the pairs inside it are scored
            _, _, g, _ = vr.fuse(np.zeros((B, K, N), np.float32), Qn, An, None, max_view_angle_deg)
            s = np.zeros((B, K, N), np.float32)
            for b in range(B):
                for k in range(K):
                    n = np.flatnonzero(g[b, k])
                    if len(n):
                        s[b, k, n] = oracle.score_hypotheses(refs[b, k][None], vq[b, k][None], Rv[b, k][n], *w)[0][0]
            S, _, _, _ = vr.fuse(s, Qn, An, None, max_view_angle_deg)
            with np.errstate(over="ignore"):
                S = S.astype(np.float32)
            key = torch.from_numpy(vr.best_keys(S))
            if best_key is not None:
                assert reset_best is True
                best_key.copy_(key)
                key = best_key
            S = torch.from_numpy(S)
            if scores_out is not None:
                scores_out.copy_(S)
                S = scores_out
            self.calls.append("verify_views_staged")
            return S, key

    return TrackViewsOracleBackend()
