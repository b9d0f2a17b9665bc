"""numpy fp64 reference of the trajectory smoother (``ahv_smooth_step_f32`` / ``ahv_smooth_backtrace_f32``, include/ahv.h): the
Viterbi recursion over a ring of particle sets and its backtrace, a brute-force path maximiser for tiny cases, the planted
sequence with two distractor frames, and the oracle-backed CPU backend of ``track.PoseTracker(history=H)``.

    viterbi_step   delta_j = a_j + max_i [(delta_i - m) + max(-|P_i - R_j|_F^2 k, -jump)], back_j = the first such i;
                   a_j = beta s_j; a non-finite s_j: dead (delta -inf, back -1); a non-finite delta_i: dead predecessor;
                   a NaN or -inf c_ij is no candidate; without a candidate delta_j = a_j, back_j = -1
    Ring           the H-slot ring with the slot arithmetic of the entry points; ``backtrace`` is the rule of the header
"""
import itertools
import math

import numpy as np

from . import track_reference as tr


def inv4s2(sigma_rad):
    """1 / (4 sigma^2) in fp64 from the fp32 sigma the entry point is given."""
    s = float(np.float32(sigma_rad))
    return 1.0 / (4.0 * s * s)


def predicted(R, V=None, damping=1.0):
    """The pose a particle predicts for the next frame, fp64: R exp([damping v]x); R itself without velocities."""
    R = np.asarray(R, dtype=np.float64)
    if V is None:
        return R
    return R @ tr.exp_so3(float(damping) * np.asarray(V, dtype=np.float64))


def transition(P_prev, R, k, jump):
    """(Mi, Mj) fp64: max(-|P_i - R_j|_F^2 k, -jump) from the nine differences; a NaN stays a NaN."""
    P_prev, R = np.asarray(P_prev, dtype=np.float64), np.asarray(R, dtype=np.float64)
    d = P_prev.reshape(-1, 1, 9) - R.reshape(1, -1, 9)
    with np.errstate(invalid="ignore", over="ignore"):
        w = -(d * d).sum(-1) * k
        return np.where(w < -jump, -jump, w)


def candidates(R, P_prev, delta_prev, k, jump):
    """(c (Mi, Mj) fp64 with -inf where i is no candidate for j, m) or (None, None) when no predecessor is alive."""
    delta_prev = np.asarray(delta_prev, dtype=np.float64)
    alive = np.isfinite(delta_prev)
    if not alive.any():
        return None, None
    m = delta_prev[alive].max()
    with np.errstate(invalid="ignore"):
        c = np.where(alive, delta_prev - m, np.nan)[:, None] + transition(P_prev, R, k, jump)
    return np.where(np.isnan(c), -np.inf, c), m


def viterbi_step(R, scores, beta, k, jump, P_prev=None, delta_prev=None):
    """One sample, one frame: (delta (M,) fp64, back (M,) int32).  R (M,3,3), scores (M,); P_prev (Mi,3,3) and delta_prev
    (Mi,), the previous slot, or None for a frame without predecessors.  beta as the fp32 the entry point is given."""
    s = np.asarray(scores, dtype=np.float64)
    ok = np.isfinite(s)
    with np.errstate(invalid="ignore", over="ignore"):
        a = float(np.float32(beta)) * s
    best, back = np.zeros(len(s)), np.full(len(s), -1, np.int32)
    c = None if delta_prev is None else candidates(R, P_prev, delta_prev, k, jump)[0]
    if c is not None:
        top = c.max(axis=0)
        has = top > -np.inf
        best = np.where(has, top, 0.0)
        back = np.where(has, c.argmax(axis=0), -1).astype(np.int32)      # argmax: the first index that attains it
    with np.errstate(invalid="ignore"):
        delta = np.where(ok, a + best, -np.inf)
    return delta, np.where(ok, back, -1).astype(np.int32)


class Ring:
    """The ring of the entry points in numpy: R, P (H,B,M,3,3) fp64, delta (H,B,M) fp64, back (H,B,M) int32.  ``fill`` sets
    what an unwritten slot holds (NaN by default: a step at first_step must read none of it)."""

    def __init__(self, H, B, M, velocities=False, fill=np.nan):
        self.H, self.B, self.M = H, B, M
        self.R = np.full((H, B, M, 3, 3), fill, np.float64)
        self.P = np.full((H, B, M, 3, 3), fill, np.float64) if velocities else None
        self.delta = np.full((H, B, M), fill, np.float64)
        self.back = np.full((H, B, M), -7, np.int32)

    def step(self, t, R, scores, beta, sigma_rad, jump, V=None, damping=1.0, first_step=1):
        assert (V is not None) == (self.P is not None)
        k = inv4s2(sigma_rad)
        slot, prev = t % self.H, (t - 1) % self.H
        R = np.asarray(R, dtype=np.float64)
        for b in range(self.B):
            if t > first_step:
                Pp = (self.P if self.P is not None else self.R)[prev, b]
                d, bk = viterbi_step(R[b], scores[b], beta, k, jump, Pp, self.delta[prev, b])
            else:
                d, bk = viterbi_step(R[b], scores[b], beta, k, jump)
            self.delta[slot, b], self.back[slot, b] = d, bk
        self.R[slot] = R
        if self.P is not None:
            self.P[slot] = predicted(R, V, damping)

    def backtrace(self, t, F, first_step=1):
        """(idx (B,F) int64, R (B,F,3,3) fp64), oldest first."""
        assert 1 <= F <= self.H
        idx = np.full((self.B, F), -1, np.int64)
        Rp = np.tile(np.eye(3), (self.B, F, 1, 1))
        for b in range(self.B):
            carry = -1
            for k in range(F):
                tk = t - k
                if tk < first_step:
                    carry = -1
                    continue
                slot = tk % self.H
                if carry < 0:
                    d = self.delta[slot, b]
                    fin = np.isfinite(d)
                    carry = int(np.argmax(np.where(fin, d, -np.inf))) if fin.any() else -1
                if carry >= 0:
                    idx[b, F - 1 - k], Rp[b, F - 1 - k] = carry, self.R[slot, b, carry]
                    nxt = int(self.back[slot, b, carry])
                    carry = nxt if 0 <= nxt < self.M else -1
        return idx, Rp


def path_value(path, Rs, Ps, scores, beta, k, jump):
    """Log-posterior of one path (a particle index per frame) of one sample, fp64; -inf through a dead particle."""
    v = 0.0
    for f, j in enumerate(path):
        s = float(scores[f][j])
        if not math.isfinite(s):
            return -np.inf
        v += float(np.float32(beta)) * s
        if f:
            w = float(transition(Ps[f - 1][path[f - 1]][None], Rs[f][j][None], k, jump)[0, 0])
            if math.isnan(w):
                return -np.inf
            v += w
    return v


def brute_force(Rs, Ps, scores, beta, k, jump):
    """The best path over every M^T sequence of one sample: (value, [paths that attain it]).  Rs, Ps: T arrays (M,3,3);
    scores: T arrays (M,).  For tiny M and T only."""
    M, T = len(scores[0]), len(scores)
    best, arg = -np.inf, []
    for path in itertools.product(range(M), repeat=T):
        v = path_value(path, Rs, Ps, scores, beta, k, jump)
        if v > best:
            best, arg = v, [path]
        elif v == best and v > -np.inf:
            arg.append(path)
    return best, arg


# ---- the planted sequence with distractor frames ---------------------------------------------------------------------
# track_reference.PLANTED (3 degrees per frame, 512 particles, sigma 3, 32 fresh slots, T = 0.02) with frames 5 and 8 replaced by
# an unrelated view of the object: vol_tgt = rotate_volume(vol_src, D), D one of three Haar rotations of seed 99 + s.
DISTRACTED = dict(tr.PLANTED, distractors=(5, 8), distractor_seed=99, history=12, smooth_sigma_deg=3.0, smooth_jump=8.0, judged=(4, 12))


def distractor(rotations, s, k):
    """The pose shown in place of frame k of sequence s, (3,3) fp64."""
    return rotations.haar_rotations_np(3, seed=DISTRACTED["distractor_seed"] + s)[k % 3].astype(np.float64)


def distracted_run(rotations, s, rotate, tracker_init, tracker_step, smoothed):
    """Planted sequence s with the distractor frames: (filter errors (12,), smoothed-path errors (11,) for frames 1..11), in
    degrees against the ground truth of the CLEAN sequence.  ``rotate(R (3,3) fp64) -> vol_tgt``; ``tracker_init(vol_tgt)`` /
    ``tracker_step(vol_tgt)`` return a TrackStep (batch 1); ``smoothed()`` returns the SmoothedPath after the last frame."""
    gt = tr.planted_truth(rotations, s)
    err = []
    for k in range(DISTRACTED["frames"]):
        vt = rotate(distractor(rotations, s, k) if k in DISTRACTED["distractors"] else gt[k])
        res = tracker_init(vt) if k == 0 else tracker_step(vt)
        err.append(float(tr.geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])))
    path = smoothed()
    Rp = path.R[0].double().cpu().numpy()
    assert Rp.shape[0] == DISTRACTED["frames"] - 1       # the frame given to init is not recorded
    return np.asarray(err), tr.geodesic_deg(Rp, gt[1:])


def distracted_bar(smooth_err, blind_err):
    """The bar: the smoothed path's largest error over frames 4-11 stays below the median of the blind 4 096-hypothesis arg-max
    error over the 12 frames of the CLEAN sequence (track_reference.planted_bar's right-hand side).  ``smooth_err`` starts at
    frame 1.  Returns (smoothed max, blind median)."""
    lo, hi = DISTRACTED["judged"]
    return float(np.max(np.asarray(smooth_err)[lo - 1:hi - 1])), float(np.median(np.asarray(blind_err)))


# ---- oracle-backed CPU backend ----------------------------------------------------------------------------------------
def make_backend(ahv, oracle, base=None):
    """``base`` (default: track_reference.make_backend's object; track_cv_reference's works too) plus ``smooth_step`` and
    ``smooth_backtrace`` with the signatures of 3dahv_amd.ops, computed by the fp64 reference on the ring's host tensors."""
    import torch

    if base is None:
        base = tr.make_backend(ahv, oracle)

    class SmoothOracleBackend(type(base)):
        def smooth_step(self, history, R, scores, step, temperature, sigma_deg, jump=8.0, V=None, damping=1.0, first_step=1):
            H, B, M = history.R.shape[:3]
            assert (V is not None) == (history.P is not None) and tuple(R.shape) == (B, M, 3, 3)
            t = int(step[0])
            slot, prev = t % H, (t - 1) % H
            beta = ahv.ops.inverse_temperature(temperature)
            k = inv4s2(math.radians(sigma_deg))
            for b in range(B):
                args = ()
                if t > first_step:
                    Pp = (history.P if history.P is not None else history.R)[prev, b].numpy()
                    args = (Pp, history.delta[prev, b].numpy())
                d, bk = viterbi_step(R[b].numpy(), scores[b].numpy(), beta, k, float(jump), *args)
                history.delta[slot, b] = torch.from_numpy(d.astype(np.float32))
                history.back[slot, b] = torch.from_numpy(bk)
            history.R[slot].copy_(R)
            if V is not None:
                history.P[slot].copy_(torch.from_numpy(predicted(R.numpy(), V.numpy(), damping).astype(np.float32)))
            self.calls.append("smooth_step")
            self.last_smooth = dict(t=t, sigma_deg=sigma_deg, jump=jump, V=V, damping=damping, first_step=first_step)
            return history

        def smooth_backtrace(self, history, step, frames=None, first_step=1, out=None):
            H, B, M = history.R.shape[:3]
            ring = Ring(H, B, M)
            ring.R, ring.delta, ring.back = history.R.double().numpy(), history.delta.double().numpy(), history.back.numpy()
            idx, Rp = ring.backtrace(int(step[0]), H if frames is None else int(frames), first_step)
            res = ahv.ops.SmoothedPath(torch.from_numpy(idx), torch.from_numpy(Rp.astype(np.float32)))
            if out is not None:
                out.idx.copy_(res.idx)
                out.R.copy_(res.R)
                res = out
            self.calls.append("smooth_backtrace")
            return res

    be = SmoothOracleBackend()
    return be
