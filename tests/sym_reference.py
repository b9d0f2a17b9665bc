"""Numpy fp64 restatement of pose selection modulo a symmetry group (include/ahv.h, "Pose selection modulo an object's symmetry
group"): the symmetric trace t_G and its maximiser, the fold of ``ahv_sym_fold_f32`` and the mode selection of
``ahv_topk_modes_sym_f32``.  Plain module (like tests/modes_reference.py).

The group acts on the right: R and R S are the same pose.  S (G,3,3) with S[0] the identity; optionally a unit axis a about which
every rotation is a symmetry too.
    t_G(R, A) = max over S of sum_ab (R S)[a][b] A[a][b]
      finite part   t_g = <R S_g, A>
      with an axis  M = A^T R S_g, p = a^T M a, c = tr M - p, s = -a . (M32 - M23, M13 - M31, M21 - M12); value_g = p + sqrt(c^2 + s^2)
                    at cos phi = c / h, sin phi = s / h (phi = 0 when h = 0)
The FIRST maximising g is kept (strict >, g ascending, starting from g = 0: a NaN value never replaces the incumbent and a NaN
value at g = 0 stays).  "Within theta" is t_G >= tau; a NaN t_G is never within.

Everything is computed in fp64 here (the kernels: fp32, any summation order).  Beside every result comes the MARGIN of the
decisions behind it -- the smaller of |t_G - tau| and the gap between the best and the second-best element -- so that a test
compares decisions only where the margin is far above what an fp32 summation order can move a trace by (~1e-6).
"""
import importlib
import math

import numpy as np

EMPTY = -(1 << 63)


def tau_of(min_angle_deg):
    """tau = 1 + 2 cos(theta): double precision, rounded to fp32; None (no limit) -> -inf."""
    if min_angle_deg is None:
        return -np.inf
    return float(np.float32(1.0 + 2.0 * math.cos(math.radians(float(min_angle_deg)))))


def rot(a, cphi, sphi):
    """Rot(a, phi) = cos I + sin [a]x + (1 - cos) a a^T for arrays cphi, sphi (n,) -> (n,3,3)."""
    a = np.asarray(a, dtype=np.float64)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    c, s = np.asarray(cphi, dtype=np.float64)[:, None, None], np.asarray(sphi, dtype=np.float64)[:, None, None]
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)


def element_values(R, A, S, axis=None):
    """R (n,3,3), A (3,3), S (G,3,3), axis (3,) or None -> (vals (n,G), c (n,G), s (n,G)): the value of every element (with an
    axis: maximised over phi) and the c, s it is reached with (1, 0 without an axis)."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    A = np.asarray(A, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        M = A.T[None, None] @ R[:, None] @ S[None]                       # (n,G,3,3) = A^T R S_g
        tr = M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2]
        if axis is None:
            return tr, np.ones_like(tr), np.zeros_like(tr)
        a = np.asarray(axis, dtype=np.float64)
        p = np.einsum("i,ngij,j->ng", a, M, a)
        c = tr - p
        s = -(a[0] * (M[..., 2, 1] - M[..., 1, 2]) + a[1] * (M[..., 0, 2] - M[..., 2, 0]) + a[2] * (M[..., 1, 0] - M[..., 0, 1]))
        return p + np.sqrt(c * c + s * s), c, s


def sym_trace(R, A, S, axis=None):
    """-> (t (n,), g (n,) int, cphi (n,), sphi (n,), gap (n,)): t_G, its first maximiser, the axis turn, and the gap between the
    best and the second-best element value (inf for G = 1, NaN-free: a NaN value counts as no competitor)."""
    vals, c, s = element_values(R, A, S, axis)
    n, G = vals.shape
    t, g = vals[:, 0].copy(), np.zeros(n, dtype=np.int64)
    for k in range(1, G):
        with np.errstate(invalid="ignore"):
            better = vals[:, k] > t
        t[better] = vals[better, k]
        g[better] = k
    idx = np.arange(n)
    cb, sb = c[idx, g], s[idx, g]
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.sqrt(cb * cb + sb * sb)
        turn = (h > 0) if axis is not None else np.zeros(n, dtype=bool)
        cphi = np.where(turn, cb / np.where(turn, h, 1.0), 1.0)
        sphi = np.where(turn, sb / np.where(turn, h, 1.0), 0.0)
    gap = np.full(n, np.inf)
    if G > 1:
        others = vals.copy()
        others[idx, g] = -np.inf
        others = np.where(np.isnan(others), -np.inf, others)
        with np.errstate(invalid="ignore"):
            gap = t - others.max(axis=1)
        gap = np.where(np.isnan(gap), np.inf, gap)
    return t, g, cphi, sphi, gap


def _per_sample(x, b, nd):
    """x with or without a leading batch axis (nd = its dimensionality without one)."""
    if x is None:
        return None
    x = np.asarray(x)
    return x[b] if x.ndim == nd + 1 else x


def fold(R, S, axis, anchors, min_angle_deg=None, keep=0, V=None):
    """R (N,3,3) | (B,N,3,3); S (G,3,3) | (B,G,3,3); axis None | (3,) | (B,3); anchors (B,K,3,3) (an all-zero anchor is an empty
    slot); V None | (B,N,3).  -> dict: R (B,N,3,3) fp64, which, elem (B,N) int, trace (B,N), V (B,N,3) or None, moved (B,N) bool
    (False where the result is the input's bytes) and margin (B,N): the smallest |t_G - tau| over the anchors examined (inf
    without a limit) and, where an anchor took the hypothesis, the element gap at that anchor."""
    anchors = np.asarray(anchors)
    B, K = anchors.shape[:2]
    tau = tau_of(min_angle_deg)
    N = np.asarray(R).shape[-3]
    out = dict(R=np.zeros((B, N, 3, 3)), which=np.full((B, N), -1, dtype=np.int64), elem=np.full((B, N), -1, dtype=np.int64),
               trace=np.full((B, N), np.nan), V=None if V is None else np.zeros((B, N, 3)), moved=np.zeros((B, N), dtype=bool),
               margin=np.full((B, N), np.inf))
    for b in range(B):
        Rb = np.asarray(_per_sample(R, b, 3), dtype=np.float64)
        Sb = np.asarray(_per_sample(S, b, 3), dtype=np.float64)
        ab = _per_sample(axis, b, 1)
        ab = None if ab is None else np.asarray(ab, dtype=np.float64)
        Vb = None if V is None else np.asarray(V[b], dtype=np.float64)
        out["R"][b] = Rb
        if V is not None:
            out["V"][b] = Vb
        open_ = np.arange(N) >= keep
        for k in range(K):
            if not np.any(np.asarray(anchors[b, k]) != 0):   # an empty slot (a NaN entry is "used")
                continue
            live = np.flatnonzero(open_)
            if live.size == 0:
                break
            t, g, cphi, sphi, gap = sym_trace(Rb[live], anchors[b, k], Sb, ab)
            with np.errstate(invalid="ignore"):
                if np.isfinite(tau):
                    d = np.abs(t - tau)
                    d = np.where(np.isnan(d), np.inf, d)
                    out["margin"][b, live] = np.minimum(out["margin"][b, live], d)
                hit = t >= tau
            idx = live[hit]
            out["which"][b, idx], out["elem"][b, idx], out["trace"][b, idx] = k, g[hit], t[hit]
            out["margin"][b, idx] = np.minimum(out["margin"][b, idx], gap[hit])
            moved = (g[hit] != 0) | (~((sphi[hit] == 0) & (cphi[hit] > 0)) if ab is not None else np.zeros(idx.size, dtype=bool))
            Q = Sb[g[hit]] @ (rot(ab, cphi[hit], sphi[hit]) if ab is not None else np.eye(3)[None])
            out["R"][b, idx] = np.where(moved[:, None, None], Rb[idx] @ Q, Rb[idx])
            if V is not None:
                out["V"][b, idx] = np.where(moved[:, None], np.einsum("nij,ni->nj", Q, Vb[idx]), Vb[idx])
            out["moved"][b, idx] = moved
            open_[idx] = False
    return out


def select_modes(scores, R, K, min_angle_deg, S, axis=None, n_offset=0):
    """tests/modes_reference.select_modes with "alive i dies when t_G(R_i, R_w) >= tau".  S (G,3,3) | (B,G,3,3), axis None | (3,) |
    (B,3).  -> (keys (B,K) int64 EMPTY-padded, margin): the smallest |t_G - tau| over every (round, alive hypothesis other than the
    winner) decision, inf when none was made."""
    pack = importlib.import_module("3dahv_amd").dist.pack_keys_host
    scores = np.asarray(scores, dtype=np.float32)
    B, N = scores.shape
    tau = tau_of(min_angle_deg)
    keys = np.full((B, K), EMPTY, dtype=np.int64)
    margin = np.inf
    for b in range(B):
        Rb = np.asarray(_per_sample(R, b, 3), dtype=np.float64)
        Sb = np.asarray(_per_sample(S, b, 3), dtype=np.float64)
        ab = _per_sample(axis, b, 1)
        cand = pack(scores[b], np.arange(N, dtype=np.int64) + n_offset).reshape(N)
        alive = np.ones(N, dtype=bool)
        for j in range(K):
            if not alive.any():
                break
            live = np.flatnonzero(alive)
            w = live[np.argmax(cand[live])]
            keys[b, j] = cand[w]
            alive[w] = False                      # by index
            live = np.flatnonzero(alive)
            if live.size == 0:
                continue
            t = sym_trace(Rb[live], Rb[w], Sb, ab)[0]
            with np.errstate(invalid="ignore"):
                d = np.abs(t - tau)
                ok = ~np.isnan(d)
                if ok.any():
                    margin = min(margin, float(d[ok].min()))
                alive[live[t >= tau]] = False     # false for a NaN t_G
    return keys, margin


def indices(keys):
    """(B,K) keys -> global indices, -1 for EMPTY."""
    return importlib.import_module("3dahv_amd").dist.unpack_keys_host(np.asarray(keys))[1]
