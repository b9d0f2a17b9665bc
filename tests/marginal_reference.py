"""numpy fp64 reference of the marginal smoother (``ahv_marginal_step_f32`` / ``ahv_marginal_smooth_f32``, include/ahv.h): the
forward and backward sum-product recursions over the ring of tests/smooth_reference.py and the finish, brute-force marginals
over every path for tiny cases, and the oracle-backed CPU backend of ``track.PoseTracker(history=H, marginals=True)``.

    forward_step   alpha_j = a_j + LSE_i[(alpha_i - m) + w_ij] over the alive i with a non-NaN w_ij; a_j = beta s_j; a non-finite
                   s_j: dead (alpha = emit = -inf); no alive predecessor (or none given): alpha_j = a_j; alive predecessors but no
                   edge to j: alpha_j = -inf
    backward_step  beta_i = LSE_j[w_ij + (g_j - m')], g = emit + beta of the next frame; no finite g: beta_i = 0
    MarginalRing   alpha, emit (H,B,M) beside a smooth_reference.Ring; ``smooth`` is the rule of the header
"""
import collections
import itertools
import math

import numpy as np

from . import smooth_reference as sm


def lse(x, axis=0):
    """log sum exp over ``axis`` in fp64; -inf entries take no part, a slice without a finite entry gives -inf."""
    x = np.asarray(x, dtype=np.float64)
    top = np.max(x, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        out = np.log(np.sum(np.exp(x - safe), axis=axis, keepdims=True)) + safe
    return np.squeeze(out, axis=axis)


def edges(weight, w):
    """(Mi, Mj): weight_i + w_ij where weight_i is finite and the sum is not NaN, else -inf (no edge)."""
    weight = np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isfinite(weight), weight, np.nan)[:, None] + w
    return np.where(np.isnan(c), -np.inf, c)


def forward_step(R, scores, beta, k, jump, P_prev=None, alpha_prev=None):
    """One sample, one frame: (alpha (M,), emit (M,)) fp64.  P_prev (Mi,3,3) and alpha_prev (Mi,): the previous slot, or None
    for a frame without predecessors.  beta as the fp32 the entry point is given."""
    s = np.asarray(scores, dtype=np.float64)
    ok = np.isfinite(s)
    with np.errstate(invalid="ignore", over="ignore"):
        emit = np.where(ok, float(np.float32(beta)) * s, -np.inf)
    if alpha_prev is None:
        return emit.copy(), emit
    alpha_prev = np.asarray(alpha_prev, dtype=np.float64)
    alive = np.isfinite(alpha_prev)
    if not alive.any():
        return emit.copy(), emit
    m = alpha_prev[alive].max()
    c = edges(np.where(alive, alpha_prev - m, np.nan), sm.transition(P_prev, R, k, jump))
    return np.where(ok, emit + lse(c, axis=0), -np.inf), emit


def backward_step(P, R_next, g_next, k, jump):
    """beta (Mi,) fp64 of a frame from the next one: P (Mi,3,3) the frame's predicted poses, R_next (Mj,3,3) and g_next (Mj,) =
    emit + beta of the next frame."""
    g_next = np.asarray(g_next, dtype=np.float64)
    alive = np.isfinite(g_next)
    if not alive.any():
        return np.zeros(len(P))
    m = g_next[alive].max()
    w = sm.transition(P, R_next, k, jump)                                   # (Mi, Mj)
    return lse(edges(np.where(alive, g_next - m, np.nan), w.T), axis=0)    # edges wants the weighted index first


def finish(alpha, beta):
    """(log gamma (M,), idx): x = alpha + beta, log gamma = x - LSE x, -inf for a dead particle; the first arg-max, -1 and a row
    of -inf without a finite x."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(alpha, np.float64) + np.asarray(beta, np.float64)
    x = np.where(np.isfinite(x), x, -np.inf)
    if not np.isfinite(x).any():
        return np.full(len(x), -np.inf), -1
    lg = x - lse(x)
    return lg, int(np.argmax(lg))


class MarginalRing:
    """alpha, emit (H,B,M) fp64 beside ``ring`` (a smooth_reference.Ring, which records R and P): ``step`` is the forward step of
    frame t (ring.step(t - 1, ...) must have run; ring.step(t, ...) may run before or after), ``smooth`` the query."""

    def __init__(self, ring, fill=np.nan):
        self.ring = ring
        self.alpha = np.full((ring.H, ring.B, ring.M), fill, np.float64)
        self.emit = np.full((ring.H, ring.B, ring.M), fill, np.float64)

    def step(self, t, R, scores, beta, sigma_rad, jump, first_step=1):
        ring = self.ring
        k = sm.inv4s2(sigma_rad)
        slot, prev = t % ring.H, (t - 1) % ring.H
        R = np.asarray(R, dtype=np.float64)
        for b in range(ring.B):
            args = ()
            if t > first_step:
                args = ((ring.P if ring.P is not None else ring.R)[prev, b], self.alpha[prev, b].copy())
            self.alpha[slot, b], self.emit[slot, b] = forward_step(R[b], scores[b], beta, k, jump, *args)

    def smooth(self, t, F, sigma_rad, jump, first_step=1):
        """(logw (B,F,M), idx (B,F) int64, R (B,F,3,3)) fp64, oldest first."""
        ring = self.ring
        assert 1 <= F <= ring.H
        k = sm.inv4s2(sigma_rad)
        logw = np.full((ring.B, F, ring.M), -np.inf)
        idx = np.full((ring.B, F), -1, np.int64)
        Rp = np.tile(np.eye(3), (ring.B, F, 1, 1))
        for b in range(ring.B):
            beta = np.zeros(ring.M)
            for back in range(F):
                tau = t - back
                if tau < first_step:
                    break
                slot = tau % ring.H
                logw[b, F - 1 - back], j = finish(self.alpha[slot, b], beta)
                if j >= 0:
                    idx[b, F - 1 - back], Rp[b, F - 1 - back] = j, ring.R[slot, b, j]
                if tau - 1 >= first_step:
                    prev = (tau - 1) % ring.H
                    with np.errstate(invalid="ignore"):
                        g = self.emit[slot, b] + beta
                    beta = backward_step((ring.P if ring.P is not None else ring.R)[prev, b], ring.R[slot, b], g, k, jump)
        return logw, idx, Rp


def brute_force_marginals(Rs, Ps, scores, beta, k, jump):
    """log gamma per frame, a list of T arrays (M,), from all M^T paths of one sample (smooth_reference.path_value).  For tiny M
    and T only, and for sequences in which every frame has a particle on a path of finite value."""
    M, T = len(scores[0]), len(scores)
    paths = list(itertools.product(range(M), repeat=T))
    v = np.array([sm.path_value(p, Rs, Ps, scores, beta, k, jump) for p in paths])
    assert np.isfinite(v).any()
    total = lse(v)
    out = []
    for f in range(T):
        col = np.array([p[f] for p in paths])
        out.append(np.array([lse(np.where(col == i, v, -np.inf)) - total for i in range(M)]))
    return out


# ---- oracle-backed CPU backend ----------------------------------------------------------------------------------------
Posterior = collections.namedtuple("Posterior", ["R_mean", "spread_deg", "mode_prob", "entropy"])


def make_backend(ahv, oracle, base=None):
    """smooth_reference.make_backend(ahv, oracle, base) plus ``marginal_step`` and ``marginal_smooth`` with the signatures of
    3dahv_amd.ops, computed by the fp64 reference on the rings' host tensors, and ``pose_posterior`` (the fields the tracker
    reads) by tests/posterior_reference.py."""
    import torch

    from . import posterior_reference as pr

    base = sm.make_backend(ahv, oracle, base)

    def rings(history, marg):
        H, B, M = history.R.shape[:3]
        ring = sm.Ring(H, B, M, velocities=history.P is not None)
        ring.R = history.R.double().numpy()
        if history.P is not None:
            ring.P = history.P.double().numpy()
        mr = MarginalRing(ring)
        mr.alpha, mr.emit = marg.alpha.double().numpy(), marg.emit.double().numpy()
        return mr

    class MarginalOracleBackend(type(base)):
        def marginal_step(self, history, marg, R, scores, step, temperature, sigma_deg, jump=8.0, first_step=1):
            assert isinstance(marg, ahv.ops.MarginalHistory) and tuple(marg.alpha.shape) == tuple(history.R.shape[:3])
            t = int(step[0])
            mr = rings(history, marg)
            mr.step(t, R.numpy(), scores.numpy(), ahv.ops.inverse_temperature(temperature), math.radians(sigma_deg), float(jump),
                    first_step)
            slot = t % history.R.shape[0]
            marg.alpha[slot] = torch.from_numpy(mr.alpha[slot].astype(np.float32))
            marg.emit[slot] = torch.from_numpy(mr.emit[slot].astype(np.float32))
            self.calls.append("marginal_step")
            self.last_marginal = dict(t=t, sigma_deg=sigma_deg, jump=jump, first_step=first_step)
            return marg

        def marginal_smooth(self, history, marg, step, sigma_deg, jump=8.0, frames=None, first_step=1, out=None):
            H = history.R.shape[0]
            logw, idx, Rp = rings(history, marg).smooth(int(step[0]), H if frames is None else int(frames), math.radians(sigma_deg),
                                                        float(jump), first_step)
            res = ahv.ops.SmoothedMarginals(torch.from_numpy(logw.astype(np.float32)), torch.from_numpy(idx),
                                            torch.from_numpy(Rp.astype(np.float32)))
            if out is not None:
                for dst, src in zip(out, res):
                    dst.copy_(src)
                res = out
            self.calls.append("marginal_smooth")
            return res

        def pose_posterior(self, scores, R, temperature=0.1, anchors=None, min_angle_deg=None, **kw):
            got, _ = pr.posterior(scores.numpy(), R.numpy(), None if anchors is None else anchors.numpy(), min_angle_deg, temperature)
            f = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32))
            self.calls.append("pose_posterior")
            return Posterior(f(got["R_mean"]), f(got["spread_deg"]), f(got["mode_prob"]), f(got["entropy"]))

    return MarginalOracleBackend()
