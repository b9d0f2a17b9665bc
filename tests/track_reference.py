"""numpy fp64 reference of the tracker's predict step (``ahv_diffuse_rotations_f32``, include/ahv.h), a mirror of one filter
step that takes its random numbers as arguments, the planted moving optimum both test tiers track, and the oracle-backed CPU
backend of ``track.PoseTracker``.

    diffuse     out[b][j] = R[b][idx[b][j]] exp([omega[b][j]]x); slot 0 = R[b][best_idx[b]] when best_idx is given; the last
                fresh.shape[1] slots = fresh; an index outside [0, N) reads row 0
"""
import math

import numpy as np

from . import resample_reference as rr

FRESH_SEED_XOR = 0x9E3779B97F4A7C15


def exp_so3(omega):
    """Rodrigues in fp64: (..., 3) rotation vectors -> (..., 3, 3); 1 - cos a as 2 sin^2(a/2), series below 1e-8 rad."""
    w = np.asarray(omega, dtype=np.float64)
    a = np.sqrt((w * w).sum(-1))[..., None, None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    small = a < 1e-8
    safe = np.where(small, 1.0, a)
    A = np.where(small, 1.0 - a * a / 6.0, np.sin(safe) / safe)
    Bc = np.where(small, 0.5 - a * a / 24.0, 2.0 * np.sin(0.5 * safe) ** 2 / (safe * safe))
    return np.eye(3) + A * K + Bc * (K @ K)


def gather(R, idx):
    """R (N,3,3) or (B,N,3,3), idx (B,M) -> (B,M,3,3); outside [0, N): row 0."""
    R, idx = np.asarray(R), np.asarray(idx)
    N = R.shape[-3]
    loc = np.where((idx < 0) | (idx >= N), 0, idx)
    return R[np.arange(len(idx))[:, None], loc] if R.ndim == 4 else R[loc]


def diffuse(R, idx, omega, best_idx=None, fresh=None):
    """The predict step in fp64.  R (N,3,3) / (B,N,3,3), idx (B,M) int64 (None: j mod N), omega (B,M,3) as applied, best_idx
    (B,) or None (the elite of slot 0, copied), fresh (B,F,3,3) or None (the last F slots, copied)."""
    omega = np.asarray(omega, dtype=np.float64)
    B, M = omega.shape[:2]
    N = np.asarray(R).shape[-3]
    if idx is None:
        idx = np.broadcast_to(np.arange(M, dtype=np.int64) % N, (B, M))
    out = gather(np.asarray(R, dtype=np.float64), idx) @ exp_so3(omega)
    if fresh is not None and np.asarray(fresh).shape[1]:
        out[:, M - np.asarray(fresh).shape[1]:] = fresh
    if best_idx is not None:
        out[:, 0] = gather(np.asarray(R, dtype=np.float64), np.asarray(best_idx).reshape(B, 1))[:, 0]
    return out


def geodesic_deg(A, B):
    """Angle of A^T B in degrees, fp64, from the skew part too (accurate near 0 where arccos is not)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    D = np.swapaxes(A, -1, -2) @ B
    c = (np.trace(D, axis1=-2, axis2=-1) - 1.0) / 2.0
    s = 0.5 * np.sqrt((D[..., 2, 1] - D[..., 1, 2]) ** 2 + (D[..., 0, 2] - D[..., 2, 0]) ** 2 + (D[..., 1, 0] - D[..., 0, 1]) ** 2)
    return np.degrees(np.arctan2(s, c))


def mirror_step(R_prev, scores_prev, M, temperature, u, omega, fresh=None):
    """One filter step up to the scorer, random numbers given: (draws (B,M), particles (B,M,3,3) fp64).  The elite is the
    first arg-max of the previous scores."""
    scores_prev = np.asarray(scores_prev, dtype=np.float32)
    draws = rr.resample(scores_prev, M, temperature, u)
    best = np.array([int(np.argmax(np.where(np.isnan(s), -np.inf, s))) for s in scores_prev])
    return draws, diffuse(R_prev, draws, omega, best_idx=best, fresh=fresh)


# ---- the planted moving optimum ------------------------------------------------------------------------------------
# vol_tgt(t) := rotate_volume(vol_src, R_gt(t)) makes score(R_gt(t)) = 1 the global maximum of frame t for any weights
# (tests/test_gpu_polish.py).  R_gt(t) = R_gt(0) exp(t 3deg [a]x) about the fixed axis a; 12 frames.
PLANTED = dict(frames=12, deg_per_frame=3.0, particles=512, sigma_deg=3.0, n_fresh=32, temperature=0.02, n_init=4096,
               axis=(0.48, -0.6, 0.64), gt_seed=7, init_seed=1000, late=(6, 12))


def planted_truth(rotations, s):
    """(frames,3,3) fp64 ground truths of planted sequence s: haar_rotations_np(1, seed=7+s) advanced by 3 degrees per frame."""
    R0 = rotations.haar_rotations_np(1, seed=PLANTED["gt_seed"] + s)[0].astype(np.float64)
    U, _, Vh = np.linalg.svd(R0)
    R0 = U @ Vh
    a = np.asarray(PLANTED["axis"], dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.arange(PLANTED["frames"], dtype=np.float64)[:, None]
    return R0[None] @ exp_so3(t * math.radians(PLANTED["deg_per_frame"]) * a[None])


def planted_init(rotations, s):
    """The 4 096 Haar hypotheses of init and of the per-frame blind arg-max (one set per sequence)."""
    return rotations.haar_rotations_np(PLANTED["n_init"], seed=PLANTED["init_seed"] + s)


def planted_bar(track_err, blind_err):
    """The bar of the issue: the tracker's largest error over frames 6-11 stays below the median of the blind 4 096-hypothesis
    arg-max error over the same 12 frames.  Returns (tracker max, blind median)."""
    lo, hi = PLANTED["late"]
    return float(np.max(np.asarray(track_err)[lo:hi])), float(np.median(np.asarray(blind_err)))


def planted_run(rotations, s, rotate, make_tracker, blind):
    """Planted sequence s: per-frame errors (degrees) of the tracker and of the blind 4 096-hypothesis arg-max.
    ``rotate(R_gt (3,3) fp64) -> vol_tgt``, ``blind(vol_tgt) -> R (3,3)``, ``make_tracker()`` -> an object with
    ``init_frame(vol_tgt)`` and ``step_frame(vol_tgt)`` that return a TrackStep."""
    gt = planted_truth(rotations, s)
    t = make_tracker()
    track, blind_err = [], []
    for k in range(PLANTED["frames"]):
        vt = rotate(gt[k])
        res = t.init_frame(vt) if k == 0 else t.step_frame(vt)
        track.append(float(geodesic_deg(res.R_map[0].double().cpu().numpy(), gt[k])))
        blind_err.append(float(geodesic_deg(np.asarray(blind(vt), dtype=np.float64), gt[k])))
    return track, blind_err


# ---- oracle-backed CPU backend of track.PoseTracker ------------------------------------------------------------------
def make_backend(ahv, oracle):
    """An object with the signatures of 3dahv_amd.ops for what PoseTracker calls: the CPU oracle scores, the numpy references
    resample and diffuse, numpy draws the noise (seeded by (seed, step)).  Test infrastructure: the product backend is HIP."""
    import torch

    class TrackOracleBackend:
        def __init__(self):
            self.calls = []
            self.last_omega = self.last_u = self.last_fresh = None

        def track_advance(self, step, seed, batch, u=None):
            assert u is not None and u.shape == (batch,)
            t1 = int(step[0]) + 1
            new = np.random.RandomState([seed & 0xFFFFFFFF, t1, 1]).random_sample(batch).astype(np.float32)
            u.copy_(torch.from_numpy(new))
            step[0] = t1
            self.last_u = new
            self.calls.append("track_advance")
            return u

        def resample(self, scores, m, temperature=0.1, u=None, out=None, workspace=None):
            assert out is not None
            out.copy_(torch.from_numpy(rr.resample(scores.numpy(), m, temperature, None if u is None else u.numpy())))
            self.calls.append("resample")
            return out

        def diffuse_rotations(self, R, idx=None, m=None, sigma_deg=3.0, step=None, seed=0, best_key=None, n_fresh=0,
                              max_angle_deg=None, out=None, want_omega=False, omega_out=None):
            assert out is not None and idx is not None and out.data_ptr() != R.data_ptr()
            B, M = idx.shape
            rs = np.random.RandomState([seed & 0xFFFFFFFF, int(step[0]), 2])
            omega = math.radians(sigma_deg) * rs.standard_normal((B, M, 3))
            if max_angle_deg is not None:
                a = np.linalg.norm(omega, axis=-1, keepdims=True)
                omega = omega * np.minimum(1.0, math.radians(max_angle_deg) / np.maximum(a, 1e-300))
            fresh = None
            if n_fresh:
                fresh = ahv.rotations.haar_rotations_np(B * n_fresh, seed=(seed + 77 * int(step[0])) & 0x7FFFFFFF).reshape(B, n_fresh, 3, 3)
            best = None
            if best_key is not None:
                _, best = ahv.dist.unpack_keys_host(best_key.numpy())
            omega[:, M - n_fresh:] = 0
            if best is not None:
                omega[:, 0] = 0
            new = diffuse(R.numpy(), idx.numpy(), omega, best_idx=best, fresh=fresh).astype(np.float32)
            if best is not None:   # the elite is a copy, not a product
                new[:, 0] = gather(R.numpy(), np.asarray(best).reshape(B, 1))[:, 0]
            out.copy_(torch.from_numpy(new))
            self.last_omega, self.last_fresh = omega, fresh
            self.calls.append("diffuse_rotations")
            return out

        def verify_pair(self, vol_src, vol_tgt, R, W1, W2, b2, want_scores=True, best_key=None, reset_best=None,
                        scores_out=None, **kw):
            s, best, idx = oracle.score_hypotheses(vol_src.numpy(), vol_tgt.numpy(), R.numpy(), W1.numpy(), W2.numpy(), b2.numpy())
            key = torch.from_numpy(ahv.dist.pack_keys_host(best, idx))
            if best_key is not None:
                assert reset_best is True
                best_key.copy_(key)
                key = best_key
            s = torch.from_numpy(s)
            if scores_out is not None:
                scores_out.copy_(s)
                s = scores_out
            self.calls.append("verify_pair")
            return s, key

        def select_rotation(self, key, R, n_offset=0, reset_key=False, out=None):
            score, idx = ahv.dist.unpack_keys_host(key.numpy())
            B = key.numel()
            Rb = gather(R.numpy(), np.asarray(idx).reshape(B, 1))[:, 0]
            res = (torch.from_numpy(score), torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(Rb)))
            if out is not None:
                for o, r in zip(out, res):
                    o.copy_(r)
                res = out
            self.calls.append("select_rotation")
            return res

    return TrackOracleBackend()
