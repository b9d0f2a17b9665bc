"""numpy fp64 reference of the constant-velocity predict step (``ahv_predict_rotations_f32``, include/ahv.h), the oracle-backed
CPU backend of ``track.PoseTracker(motion="constant_velocity")`` and the fast planted sequence both test tiers track.

    predict     a particle is (R, v).  else-slots: v' = damping v_i + accel (clipped to max_speed), out = R_i exp([v' + omega_p]x);
                slot 0 = (R, v) of row best_idx when best_idx is given; slot 1 = R_n exp([v_n]x), v_n with best_idx and coast;
                the last fresh.shape[1] slots = fresh with v = 0; precedence elite > coast > fresh > else
"""
import math

import numpy as np

from . import track_reference as tr


def gather_vel(V, idx):
    """V (N,3) or (B,N,3), idx (B,M) -> (B,M,3); outside [0, N): row 0 (track_reference.gather's rule)."""
    return tr.gather(np.asarray(V)[..., None], idx)[..., 0]


def predict(R, V, idx, omega_p, accel, damping=1.0, best_idx=None, coast=True, fresh=None, max_speed=None):
    """The constant-velocity predict step in fp64: (out (B,M,3,3), vel_out (B,M,3), omega (B,M,3)).  R (N,3,3) / (B,N,3,3), V
    (N,3) / (B,N,3) or None (zeros), idx (B,M) int64 (None: j mod N), omega_p (B,M,3) the pose noise as applied, accel (B,M,3)
    the velocity noise, best_idx (B,) or None, fresh (B,F,3,3) or None, max_speed in radians or None."""
    omega_p, accel = np.asarray(omega_p, dtype=np.float64), np.asarray(accel, dtype=np.float64)
    B, M = omega_p.shape[:2]
    R = np.asarray(R, dtype=np.float64)
    N = R.shape[-3]
    V = np.zeros((N, 3)) if V is None else np.asarray(V, dtype=np.float64)
    if idx is None:
        idx = np.broadcast_to(np.arange(M, dtype=np.int64) % N, (B, M))
    vel = damping * gather_vel(V, idx) + accel
    if max_speed is not None:
        a = np.linalg.norm(vel, axis=-1, keepdims=True)
        vel = vel * np.minimum(1.0, max_speed / np.maximum(a, 1e-300))
    omega = vel + omega_p
    out = tr.gather(R, idx) @ tr.exp_so3(omega)
    F = 0 if fresh is None else np.asarray(fresh).shape[1]
    if F:
        out[:, M - F:], vel[:, M - F:], omega[:, M - F:] = fresh, 0.0, 0.0
    if best_idx is not None:
        best = np.asarray(best_idx).reshape(B, 1)
        Rn, vn = tr.gather(R, best)[:, 0], gather_vel(V, best)[:, 0]
        if coast and M >= 2:
            out[:, 1], vel[:, 1], omega[:, 1] = Rn @ tr.exp_so3(vn), vn, vn
        out[:, 0], vel[:, 0], omega[:, 0] = Rn, vn, 0.0
    return out, vel, omega


# ---- the fast planted sequence ---------------------------------------------------------------------------------------
# track_reference.PLANTED's construction (same axis, ground-truth and init seeds), moving 9 degrees per frame: three times
# the sigma of the random walk.  16 frames; the late frames are 8..15.
FAST = dict(tr.PLANTED, frames=16, deg_per_frame=9.0, particles=256, sigma_deg=3.0, sigma_vel_deg=1.0, damping=1.0, n_fresh=16,
            temperature=0.02, late=(8, 16))


def truth(rotations, s, P):
    """(frames,3,3) fp64 ground truths of sequence s of P: track_reference.planted_truth with P's length and speed."""
    R0 = tr.planted_truth(rotations, s)[0]
    a = np.asarray(P["axis"], dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.arange(P["frames"], dtype=np.float64)[:, None]
    return R0[None] @ tr.exp_so3(t * math.radians(P["deg_per_frame"]) * a[None])


def run(rotations, s, P, rotate, trackers):
    """Sequence s of P for every entry of ``trackers`` on the same frames: name -> per-frame errors in degrees.
    ``rotate(R_gt (3,3) fp64) -> vol_tgt``; an entry is a pair ``(init_frame, step_frame)`` of callables that take vol_tgt and
    return a TrackStep (batch 1)."""
    gt = truth(rotations, s, P)
    err = {name: [] for name in trackers}
    for k in range(P["frames"]):
        vt = rotate(gt[k])
        for name, (init_frame, step_frame) in trackers.items():
            res = init_frame(vt) if k == 0 else step_frame(vt)
            err[name].append(float(tr.geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])))
    return err


def fast_bar(cv_err, walk_err, P=FAST):
    """The bar of the fast sequence: the constant-velocity tracker's largest late error stays below the walk tracker's median
    late error.  Returns (cv late max, walk late median)."""
    lo, hi = P["late"]
    return float(np.max(np.asarray(cv_err)[lo:hi])), float(np.median(np.asarray(walk_err)[lo:hi]))


# ---- oracle-backed CPU backend -----------------------------------------------------------------------------------------
def make_backend(ahv, oracle):
    """track_reference.make_backend plus ``predict_rotations``: numpy draws the pose noise exactly as that backend's
    ``diffuse_rotations`` does for the same (seed, step), the velocity noise from a second stream, and the fresh slots alike."""
    import torch

    base = tr.make_backend(ahv, oracle)

    class TrackCvOracleBackend(type(base)):
        def __init__(self):
            super().__init__()
            self.last_accel = self.last_vel = self.last_V = None

        def predict_rotations(self, R, V=None, idx=None, m=None, sigma_deg=3.0, sigma_vel_deg=1.0, damping=1.0, step=None, seed=0,
                              best_key=None, coast=True, n_fresh=0, max_angle_deg=None, max_speed_deg=None, out=None,
                              vel_out=None, want_omega=False, omega_out=None):
            assert out is not None and vel_out is not None and idx is not None and out.data_ptr() != R.data_ptr()
            assert V is None or vel_out.data_ptr() != V.data_ptr()
            B, M = idx.shape
            t = int(step[0])
            omega_p = math.radians(sigma_deg) * np.random.RandomState([seed & 0xFFFFFFFF, t, 2]).standard_normal((B, M, 3))
            accel = math.radians(sigma_vel_deg) * np.random.RandomState([seed & 0xFFFFFFFF, t, 3]).standard_normal((B, M, 3))
            if max_angle_deg is not None:
                a = np.linalg.norm(omega_p, axis=-1, keepdims=True)
                omega_p = omega_p * np.minimum(1.0, math.radians(max_angle_deg) / np.maximum(a, 1e-300))
            fresh = None
            if n_fresh:
                fresh = ahv.rotations.haar_rotations_np(B * n_fresh, seed=(seed + 77 * t) & 0x7FFFFFFF).reshape(B, n_fresh, 3, 3)
            best = None
            if best_key is not None:
                _, best = ahv.dist.unpack_keys_host(best_key.numpy())
            Vn = None if V is None else V.numpy().copy()
            new, vel, omega = predict(R.numpy(), Vn, idx.numpy(), omega_p, accel, damping, best_idx=best, coast=coast, fresh=fresh,
                                      max_speed=None if max_speed_deg is None else math.radians(max_speed_deg))
            out.copy_(torch.from_numpy(new.astype(np.float32)))
            vel_out.copy_(torch.from_numpy(vel.astype(np.float32)))
            self.last_omega, self.last_accel, self.last_fresh, self.last_vel, self.last_V = omega_p, accel, fresh, vel, Vn
            self.calls.append("predict_rotations")
            return out, vel_out

    return TrackCvOracleBackend()
