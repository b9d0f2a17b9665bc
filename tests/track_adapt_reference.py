"""Noise scale and fresh slots adapted on the device (``ahv_track_control_f32`` / ``ahv_predict_rotations_ctl_f32``,
include/ahv.h): the control rule in fp64 numpy, the same formula in stock fp32 torch (the yardstick of the GPU test), the cases
both tiers run it on, the three planted sequences with their bars, and the oracle-backed CPU backend of
``track.PoseTracker(adapt=...)``.

    control     nf = clamp(record n_fresh, 0, M); reacquired = idx >= max(M - nf, first); lost = not score >= floor;
                a = angle(P^T R[idx]), P = R[0] exp([V[0]]x); m' = (1 - rate) m + rate a^2 / 3 unless lost, reacquired or a NaN;
                sigma' = sigma_max if lost else clamp(gain sqrt(m'), sigma_min, sigma_max); sigma_vel' = sigma_vel0 sigma' / sigma0;
                n_fresh' = n_fresh_lost if lost else n_fresh0
"""
import collections
import math

import numpy as np

from . import track_cv_reference as cv
from . import track_reference as tr

WORDS = 8
LOST, REACQUIRED, UPDATED = 1, 2, 4
f32 = lambda x: float(np.float32(x))
rad32 = lambda deg: f32(math.radians(deg))          # what ops._angle_rad hands the entry points

Params = collections.namedtuple("Params", ["first", "sigma0", "sigma_vel0", "n_fresh0", "sigma_min", "sigma_max", "gain", "rate",
                                           "score_floor", "n_fresh_lost"])


def params(first=1, sigma_deg=3.0, sigma_vel_deg=1.0, n_fresh=0, sigma_min_deg=0.5, sigma_max_deg=8.0, gain=1.5, rate=0.5,
           score_floor=None, n_fresh_lost=None):
    """The by-value arguments of the entry point: radians as fp32 numbers, the floats as the fp32 the ctypes call makes of them."""
    return Params(int(first), rad32(sigma_deg), rad32(sigma_vel_deg), int(n_fresh), rad32(sigma_min_deg), rad32(sigma_max_deg),
                  f32(gain), f32(rate), -math.inf if score_floor is None else f32(score_floor),
                  int(n_fresh if n_fresh_lost is None else n_fresh_lost))


# ---- the record ------------------------------------------------------------------------------------------------------
def pack(sigma, sigma_vel, n_fresh, flags, m, a, score):
    """(B,8) int32 from per-sample values; the floats are rounded to fp32."""
    B = np.broadcast(sigma, sigma_vel, n_fresh, flags, m, a, score, np.zeros(1)).shape[0]
    rec = np.zeros((B, WORDS), np.int32)
    fl = rec.view(np.float32)
    fl[:, 0], fl[:, 1], fl[:, 4], fl[:, 5], fl[:, 6] = sigma, sigma_vel, m, a, score
    rec[:, 2], rec[:, 3] = n_fresh, flags
    return rec


def unpack(rec):
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    fl = rec.view(np.float32)
    return dict(sigma=fl[:, 0].copy(), sigma_vel=fl[:, 1].copy(), n_fresh=rec[:, 2].copy(), flags=rec[:, 3].copy(), m=fl[:, 4].copy(),
                a=fl[:, 5].copy(), score=fl[:, 6].copy())


def fresh_record(B, sigma_deg, sigma_vel_deg, n_fresh):
    """What ops.track_control_state builds: m = sigma^2 in fp32, NaN innovation and score."""
    s = np.float32(rad32(sigma_deg))
    return pack(np.full(B, s), np.full(B, rad32(sigma_vel_deg)), n_fresh, 0, np.full(B, s * s), np.nan, np.nan)


# ---- the rule in fp64 ------------------------------------------------------------------------------------------------
def angle_rad(A, B):
    """Angle of A^T B in radians, fp64, by atan2 of the skew part and the trace; NaN where an entry is."""
    return np.radians(tr.geodesic_deg(A, B))


def control(rec, R, V, idx, score, p):
    """The decision in fp64 on fp32 inputs.  rec (B,8) int32, R (B,M,3,3), V (B,M,3) or None, idx (B,) int64, score (B,) float32,
    p a Params.  Returns a dict of (B,) arrays: the fp64 ``sigma``, ``sigma_vel``, ``m``, ``a`` (NaN when not computed), the exact
    ``n_fresh``, ``flags``, ``lost``, ``reacquired``, ``updated``, and ``clamped`` (-1 low, +1 high, 0 not; +1 when lost)."""
    old = unpack(rec)
    R = np.asarray(R, dtype=np.float64)
    B, M = R.shape[:2]
    idx = np.asarray(idx, dtype=np.int64)
    score = np.asarray(score, dtype=np.float32)
    nf = np.clip(old["n_fresh"].astype(np.int64), 0, M)
    reacq = idx >= np.maximum(M - nf, p.first)
    with np.errstate(invalid="ignore"):
        lost = ~(score >= np.float32(p.score_floor))
    P = R[:, 0] if V is None else R[:, 0] @ tr.exp_so3(np.asarray(V, dtype=np.float64)[:, 0])
    inside = (idx >= 0) & (idx < M)
    W = R[np.arange(B), np.where(inside, idx, 0)]
    with np.errstate(invalid="ignore"):
        a = np.where(inside, angle_rad(P, W), np.nan)
    a = np.where(np.isfinite(a), a, np.nan)
    updated = ~lost & ~reacq & np.isfinite(a)
    m_old = old["m"].astype(np.float64)
    m = np.where(updated, (1.0 - p.rate) * m_old + p.rate * np.where(updated, a, 0.0) ** 2 / 3.0, m_old)
    raw = p.gain * np.sqrt(m)
    sigma = np.where(lost, p.sigma_max, np.clip(np.where(np.isnan(raw), p.sigma_min, raw), p.sigma_min, p.sigma_max))
    clamped = np.where(lost | (raw >= p.sigma_max), 1, np.where((raw <= p.sigma_min) | np.isnan(raw), -1, 0))
    return dict(sigma=sigma, sigma_vel=p.sigma_vel0 * (sigma / p.sigma0), n_fresh=np.where(lost, p.n_fresh_lost, p.n_fresh0), m=m, a=a,
                flags=lost * LOST + reacq * REACQUIRED + updated * UPDATED, lost=lost, reacquired=reacq, updated=updated,
                clamped=clamped, raw=raw, score=score)


def control_record(rec, R, V, idx, score, p):
    """``control`` rounded into the next record: ((B,8) int32, reacquired (B,) bool)."""
    c = control(rec, R, V, idx, score, p)
    return pack(c["sigma"], c["sigma_vel"], c["n_fresh"], c["flags"], c["m"], c["a"], c["score"]), c["reacquired"]


# ---- the same formula in stock fp32 torch (CPU) ------------------------------------------------------------------------
def control_stock32(rec, R, V, idx, score, p):
    """sigma, sigma_vel, m, a (B,) float32 tensors from the formula of include/ahv.h written with stock torch operators in fp32:
    Shepperd's branch, q(P) = normalise(q(R[0]) q(V[0])) through its matrix, q = conj(q(P)) q(R[idx]), a = 2 atan2(|q_v|, |q_w|).
    The flags are taken from ``control`` (they are exact on both sides)."""
    import torch
    ref = control(rec, R, V, idx, score, p)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    c = lambda x: torch.tensor(x, dtype=torch.float32)
    R = t(R)
    B, M = R.shape[:2]

    def shepperd(r):
        r = r.reshape(-1, 9)
        r0, r1, r2, r3, r4, r5, r6, r7, r8 = r.unbind(-1)
        trc = r0 + r4 + r8
        out = []
        s = 2.0 * torch.sqrt(trc + 1.0)
        out.append(torch.stack([0.25 * s, (r7 - r5) / s, (r2 - r6) / s, (r3 - r1) / s], -1))
        s = 2.0 * torch.sqrt(1.0 + r0 - r4 - r8)
        out.append(torch.stack([(r7 - r5) / s, 0.25 * s, (r1 + r3) / s, (r2 + r6) / s], -1))
        s = 2.0 * torch.sqrt(1.0 + r4 - r0 - r8)
        out.append(torch.stack([(r2 - r6) / s, (r1 + r3) / s, 0.25 * s, (r5 + r7) / s], -1))
        s = 2.0 * torch.sqrt(1.0 + r8 - r0 - r4)
        out.append(torch.stack([(r3 - r1) / s, (r2 + r6) / s, (r5 + r7) / s, 0.25 * s], -1))
        which = torch.where(trc > 0, 0, torch.where((r0 > r4) & (r0 > r8), 1, torch.where(r4 > r8, 2, 3)))
        return torch.stack(out, 1)[torch.arange(len(r)), which]

    def hamilton(p_, q_):
        pr, pi, pj, pk = p_.unbind(-1)
        qr, qi, qj, qk = q_.unbind(-1)
        return torch.stack([pr * qr - pi * qi - pj * qj - pk * qk, pr * qi + pi * qr + pj * qk - pk * qj,
                            pr * qj - pi * qk + pj * qr + pk * qi, pr * qk + pi * qj - pj * qi + pk * qr], -1)

    qP = shepperd(R[:, 0])
    if V is not None:
        v = t(V)[:, 0]
        ang = torch.sqrt((v * v).sum(-1))
        k = torch.where(ang < 1e-3, 0.5 - ang * ang * (1.0 / 48.0), torch.sin(0.5 * ang) / ang.clamp_min(1e-30))
        q = hamilton(qP, torch.cat([torch.cos(0.5 * ang)[:, None], k[:, None] * v], -1))
        q = q / torch.sqrt((q * q).sum(-1, keepdim=True).clamp_min(1e-30))
        w, x, y, z = q.unbind(-1)
        Pm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                          2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                          2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)
        qP = shepperd(Pm)
    idx = np.asarray(idx, dtype=np.int64)
    inside = (idx >= 0) & (idx < M)
    qW = shepperd(R[torch.arange(B), torch.from_numpy(np.where(inside, idx, 0))])
    pr, pi, pj, pk = qP.unbind(-1)
    wr, wi, wj, wk = qW.unbind(-1)
    # conj(q(P)) q(R[idx]), the vector part as differences of paired products: exactly 0 for equal factors
    rel = torch.stack([pr * wr + pi * wi + pj * wj + pk * wk, (pr * wi - pi * wr) + (pk * wj - pj * wk),
                       (pr * wj - pj * wr) + (pi * wk - pk * wi), (pr * wk - pk * wr) + (pj * wi - pi * wj)], -1)
    a = 2.0 * torch.atan2(torch.sqrt((rel[:, 1:] * rel[:, 1:]).sum(-1)), rel[:, 0].abs())
    a = torch.where(torch.from_numpy(inside) & torch.isfinite(a), a, c(float("nan")))
    m_old = torch.from_numpy(unpack(rec)["m"])
    upd = torch.from_numpy(ref["updated"])
    m = torch.where(upd, (1.0 - c(p.rate)) * m_old + c(p.rate) * (torch.where(upd, a, c(0.0)) ** 2 * c(1.0 / 3.0)), m_old)
    sigma = torch.where(torch.from_numpy(ref["lost"]), c(p.sigma_max), (c(p.gain) * torch.sqrt(m)).clamp(p.sigma_min, p.sigma_max))
    return dict(sigma=sigma, sigma_vel=c(p.sigma_vel0) * (sigma / c(p.sigma0)), m=m, a=a)


# ---- the cases of the control kernel -------------------------------------------------------------------------------------
ANGLES_DEG = (0.0, 1e-3, 1.0, 170.0)                      # innovation classes
M_SIGMAS_DEG = (0.1, 2.0, 10.0)                           # sqrt(m): clamps low, does not clamp, clamps high (with a small a)
FLOOR = 0.8
SCORES = ("above", "floor", "below", "nan", "inf")        # 0.9; the floor itself (not lost); the next float below (lost); NaN; +inf
SLOTS = ("inside", "at", "under", "minus", "M", "zero")   # ordinary slot; exactly max(M - nf, first); one below; -1; M; slot 0
NEAR = 1e-3                                               # no input this close (relative) to a threshold unless deliberate


def control_case(rot, B, M, first, with_V, seed=0):
    """One launch (``rot``: the package's ``rotations`` module): a dict with ``rec, R, V, idx, score`` (numpy, fp32 / int), ``p`` (Params) and, per sample, its classes
    ``angle, slot, score_class`` (indices into the tuples above; ``angle`` -1 where the winner is slot 0 or out of range)."""
    rs = np.random.RandomState(1000 * seed + 10 * M + B)
    p = params(first=first, sigma_deg=3.0, sigma_vel_deg=1.0 if with_V else 0.0, n_fresh=min(3, M), score_floor=FLOOR,
               n_fresh_lost=M)
    R = rot.haar_rotations_np(B * M, seed=31 + seed + M).reshape(B, M, 3, 3).astype(np.float32)
    V = (math.radians(5.0) * rs.standard_normal((B, M, 3))).astype(np.float32) if with_V else None
    fresh_opts = (-1, 0, 1, min(3, M), M - 1, M, M + 5)
    b = np.arange(B)
    k_a, k_m, k_s, k_i = b % 4, (b // 4) % 3, (b // 12) % 5, (b // 60 + b) % 6
    n_fresh = np.array([fresh_opts[i] for i in (b % 7)], np.int64)
    nf = np.clip(n_fresh, 0, M)
    thr = np.maximum(M - nf, first)
    inside_slot = np.where(thr > 2, np.minimum(1 + b % max(M - 1, 1), thr - 1), min(1, M - 1))
    idx = np.select([k_i == 0, k_i == 1, k_i == 2, k_i == 3, k_i == 4], [inside_slot, thr, thr - 1, -1, M], 0).astype(np.int64)
    score = np.select([k_s == 0, k_s == 1, k_s == 2, k_s == 3], [0.9, np.float32(FLOOR), np.nextafter(np.float32(FLOOR), np.float32(-1)),
                                                                np.nan], np.inf).astype(np.float32)
    P = R[:, 0].astype(np.float64) if V is None else R[:, 0].astype(np.float64) @ tr.exp_so3(V[:, 0].astype(np.float64))
    axis = rs.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    target = P @ tr.exp_so3(np.radians(np.asarray(ANGLES_DEG))[k_a][:, None] * axis)
    movable = (idx > 0) & (idx < M)
    R[b[movable], idx[movable]] = target[movable].astype(np.float32)
    nan_row = movable & (b % 50 == 17)
    R[b[nan_row], idx[nan_row]] = np.nan
    rec = pack(rad32(3.0), rad32(1.0) if with_V else 0.0, n_fresh, 0, np.radians(np.asarray(M_SIGMAS_DEG))[k_m] ** 2, np.nan, np.nan)
    return dict(rec=rec, R=R, V=V, idx=idx, score=score, p=p, angle=np.where(movable & ~nan_row, k_a, -1), slot=k_i, score_class=k_s,
                nan_row=nan_row, thr=thr, B=B, M=M)


def control_cases(rot):
    """B = 1, 3 and 257 (the first B past one workgroup of samples) at M = 40, with and without V; M = 1 (first = 1) and M = 2
    (first = 2, with V: a coast slot)."""
    return [control_case(rot, B, 40, first, with_V, seed) for seed, (B, first, with_V) in
            enumerate(((1, 1, False), (3, 2, True), (257, 1, False), (257, 2, True)))] + \
           [control_case(rot, 3 * 60, 1, 1, False, 7), control_case(rot, 3 * 60, 2, 2, True, 8)]


# ---- the three sequences ---------------------------------------------------------------------------------------------------
# track_reference.PLANTED's construction (axis, ground-truth and init seeds) with a speed that changes: degrees per frame, one
# entry per step (frame 0 goes to init).  256 particles, sigma 3, 16 fresh slots, T = 0.02, the random walk.
_COMMON = dict(tr.PLANTED, particles=256, sigma_deg=3.0, n_fresh=16, temperature=0.02, adapt={})
ACCEL = dict(_COMMON, name="ACCEL", increments=(1.0,) * 8 + (2.5, 4.0, 5.5, 7.0, 8.5) + (9.0,) * 8, late=(14, 22))
SETTLE = dict(_COMMON, name="SETTLE", increments=(6.0,) * 8 + (0.5,) * 10, late=(11, 19))
JUMP = dict(_COMMON, name="JUMP", increments=(1.0,) * 8 + (70.0,) + (1.0,) * 14, late=(14, 24), adapt=dict(score_floor=0.8, n_fresh_lost=128))
for _P in (ACCEL, SETTLE, JUMP):
    _P["frames"] = len(_P["increments"]) + 1


def truth(rotations, s, P):
    """(frames,3,3) fp64 ground truths of sequence s of P: planted_truth's first pose turned about PLANTED's axis by the
    running sum of P's increments."""
    R0 = tr.planted_truth(rotations, s)[0]
    a = np.asarray(P["axis"], dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.concatenate([[0.0], np.cumsum(np.asarray(P["increments"], dtype=np.float64))])[:, None]
    return R0[None] @ tr.exp_so3(np.radians(t) * a[None])


def run(rotations, s, P, rotate, trackers, frames=None):
    """Sequence s of P for every entry of ``trackers`` on the same frames: name -> (per-frame errors in degrees, per-frame sigma
    in degrees the NEXT frame uses, NaN for a tracker without ``control``).  An entry is ``(init_frame, step_frame, control)``:
    the first two take vol_tgt and return a TrackStep (batch 1), ``control`` is None or returns the decoded record."""
    gt = truth(rotations, s, P)
    err = {name: ([], []) for name in trackers}
    for k in range(P["frames"] if frames is None else frames):
        vt = rotate(gt[k])
        for name, (init_frame, step_frame, control_) in trackers.items():
            res = init_frame(vt) if k == 0 else step_frame(vt)
            err[name][0].append(float(tr.geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])))
            err[name][1].append(float(control_().sigma_deg[0]) if control_ is not None else float("nan"))
    return err


def accel_bar(adapted, fixed3, P=ACCEL):
    """(A): the adapted tracker's largest late error against the fixed sigma = 3 walk's median over the same frames."""
    lo, hi = P["late"]
    return float(np.max(np.asarray(adapted)[lo:hi])), float(np.median(np.asarray(fixed3)[lo:hi]))


def settle_bar(adapted, fixed6, P=SETTLE):
    """(B): the adapted tracker's mean late error against the fixed sigma = 6 walk's, and its largest error after frame 2."""
    lo, hi = P["late"]
    return float(np.mean(np.asarray(adapted)[lo:hi])), float(np.mean(np.asarray(fixed6)[lo:hi])), float(np.max(np.asarray(adapted)[3:]))


def jump_bar(adapted, fixed3, P=JUMP):
    """(C): the largest late errors of the adapted tracker and of the fixed sigma = 3, 16-fresh one; the bar is 5 degrees."""
    lo, hi = P["late"]
    return float(np.max(np.asarray(adapted)[lo:hi])), float(np.max(np.asarray(fixed3)[lo:hi]))


JUMP_BAR_DEG = 5.0


# ---- oracle-backed CPU backend ---------------------------------------------------------------------------------------------
def make_backend(ahv, oracle):
    """track_cv_reference.make_backend plus ``predict_rotations_controlled`` and ``track_control``.  The predict step draws from
    the streams of that backend's ``diffuse_rotations`` / ``predict_rotations`` for the same (seed, step) -- the pose noise, the
    velocity noise, the fresh rotations -- and scales them per sample by the record's fp32 radians, so a record that holds
    math.radians(sigma_deg) exactly reproduces those ops bit for bit.  The control step is ``control_record``."""
    import torch

    base = cv.make_backend(ahv, oracle)

    class TrackAdaptOracleBackend(type(base)):
        def __init__(self):
            super().__init__()
            self.last_record = None

        def predict_rotations_controlled(self, R, control, V=None, idx=None, m=None, damping=1.0, step=None, seed=0, best_key=None,
                                         coast=False, max_angle_deg=None, max_speed_deg=None, out=None, vel_out=None,
                                         velocities=True, want_omega=False, omega_out=None):
            assert out is not None and idx is not None and out.data_ptr() != R.data_ptr()
            assert velocities == (vel_out is not None) and (velocities or (V is None and not coast))
            B, M = idx.shape
            t = int(step[0])
            old = unpack(control.numpy())
            self.last_record = control.numpy().copy()
            sig, sig_v = old["sigma"].astype(np.float64), old["sigma_vel"].astype(np.float64)
            nf = np.clip(old["n_fresh"].astype(np.int64), 0, M)
            omega_p = sig[:, None, None] * np.random.RandomState([seed & 0xFFFFFFFF, t, 2]).standard_normal((B, M, 3))
            if max_angle_deg is not None:
                a = np.linalg.norm(omega_p, axis=-1, keepdims=True)
                omega_p = omega_p * np.minimum(1.0, math.radians(max_angle_deg) / np.maximum(a, 1e-300))
            accel = sig_v[:, None, None] * np.random.RandomState([seed & 0xFFFFFFFF, t, 3]).standard_normal((B, M, 3)) if velocities else None
            nmax = int(nf.max())
            fresh = None
            if nmax:   # sample b takes the first nf[b] rotations of its row: the base backend's when every sample has nmax
                fresh = ahv.rotations.haar_rotations_np(B * nmax, seed=(seed + 77 * t) & 0x7FFFFFFF).reshape(B, nmax, 3, 3)
            best = None
            if best_key is not None:
                _, best = ahv.dist.unpack_keys_host(best_key.numpy())
            Rn, Vn = R.numpy(), None if V is None else V.numpy().copy()
            for b in range(B):
                Rb = Rn[b:b + 1] if Rn.ndim == 4 else Rn
                Vb = Vn[b:b + 1] if Vn is not None and Vn.ndim == 3 else Vn
                fb = fresh[b:b + 1, :nf[b]] if nf[b] else None
                bb = None if best is None else np.asarray(best)[b:b + 1]
                if velocities:
                    new, vel, _ = cv.predict(Rb, Vb, idx.numpy()[b:b + 1], omega_p[b:b + 1], accel[b:b + 1], damping,
                                             best_idx=bb, coast=coast, fresh=fb,
                                             max_speed=None if max_speed_deg is None else math.radians(max_speed_deg))
                    vel_out[b:b + 1].copy_(torch.from_numpy(vel.astype(np.float32)))
                else:   # as the base diffuse_rotations: no noise in the elite and fresh slots, the elite a copy
                    om = omega_p[b:b + 1].copy()
                    om[:, M - nf[b]:] = 0
                    if bb is not None:
                        om[:, 0] = 0
                    new = tr.diffuse(Rb, idx.numpy()[b:b + 1], om, best_idx=bb, fresh=fb).astype(np.float32)
                    if bb is not None:
                        new[:, 0] = tr.gather(Rb, bb.reshape(1, 1))[:, 0]
                    omega_p[b:b + 1] = om
                out[b:b + 1].copy_(torch.from_numpy(new.astype(np.float32)))
            self.last_omega, self.last_accel, self.last_fresh, self.last_V = omega_p, accel, fresh, Vn
            self.calls.append("predict_rotations_controlled")
            return (out, vel_out) if velocities else out

        def track_control(self, control, R, idx, score, V=None, first=1, sigma_deg=3.0, sigma_vel_deg=1.0, n_fresh=0,
                          sigma_min_deg=0.5, sigma_max_deg=8.0, gain=1.5, rate=0.5, score_floor=None, n_fresh_lost=None,
                          reacquired=None):
            assert reacquired is not None and reacquired.dtype == torch.bool
            p = params(first, sigma_deg, sigma_vel_deg, n_fresh, sigma_min_deg, sigma_max_deg, gain, rate, score_floor, n_fresh_lost)
            rec, reacq = control_record(control.numpy(), R.numpy(), None if V is None else V.numpy(), idx.numpy(), score.numpy(), p)
            control.copy_(torch.from_numpy(rec))
            reacquired.copy_(torch.from_numpy(reacq))
            self.calls.append("track_control")
            return reacquired

    return TrackAdaptOracleBackend()
