"""Numpy restatement of the mode selection of ``ahv_topk_modes_f32`` (include/ahv.h, "Distinct pose modes").  Plain module
(like tests/rotation_families.py).

For each sample, entries j = 0 .. K-1 in order: the largest packed key (``dist.pack_keys_host``: signed int64 order = NaN
first, lowest index among equal scores, -0 = +0) among the hypotheses still alive, EMPTY when none is; the winner w leaves
the alive set by its index, unconditionally, and so does every alive i with t(i, w) = sum_ab R_i[a][b] R_w[a][b] >= tau.  A
NaN t removes nothing.  t is computed in fp64 here (the kernel: fp32, any summation order), and the smallest |t - tau| over
every decision made is returned beside the list: a test compares lists only where that margin is far above what an fp32
summation-order difference can move t by (~1e-6), so that the kernel's fp32 t cannot flip a decision.
"""
import importlib
import math

import numpy as np

EMPTY = -(1 << 63)


def tau_of(min_angle_deg):
    """tau = 1 + 2 cos(theta): double precision, rounded to fp32 (what the host passes to the kernel)."""
    return np.float32(1.0 + 2.0 * math.cos(math.radians(float(min_angle_deg))))


def select_modes(scores, R, K, min_angle_deg, n_offset=0):
    """scores (B,N) fp32, R (N,3,3) or (B,N,3,3) -> (keys (B,K) int64 EMPTY-padded, margin): margin = the smallest
    |t - tau| over every (round, alive hypothesis other than the winner) decision, inf when none was made."""
    pack = importlib.import_module("3dahv_amd").dist.pack_keys_host
    scores = np.asarray(scores, dtype=np.float32)
    B, N = scores.shape
    tau = float(tau_of(min_angle_deg))
    keys = np.full((B, K), EMPTY, dtype=np.int64)
    margin = np.inf
    for b in range(B):
        Rb = np.asarray(R[b] if np.ndim(R) == 4 else R, dtype=np.float64).reshape(N, 9)
        cand = pack(scores[b], np.arange(N, dtype=np.int64) + n_offset).reshape(N)
        alive = np.ones(N, dtype=bool)
        for j in range(K):
            if not alive.any():
                break
            live = np.flatnonzero(alive)
            w = live[np.argmax(cand[live])]
            keys[b, j] = cand[w]
            alive[w] = False                      # by index: t(w, w) may be below tau for a non-rotation
            live = np.flatnonzero(alive)
            if live.size == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                t = Rb[live] @ Rb[w]
                d = np.abs(t - tau)
            ok = ~np.isnan(d)
            if ok.any():
                margin = min(margin, float(d[ok].min()))
            with np.errstate(invalid="ignore"):
                alive[live[t >= tau]] = False     # false for a NaN t
    return keys, margin


def indices(keys):
    """(B,K) keys -> global indices, -1 for EMPTY."""
    return importlib.import_module("3dahv_amd").dist.unpack_keys_host(np.asarray(keys))[1]
