"""The cases of tests/test_gpu_rng.py and what the host mirror (tests/rng_reference.py) computes for each, built once per
process and never modified.  tests/test_rng_cpu.py asserts the conditions each case has to meet; a seed that misses one is
stepped (seed, seed + 1, ...), as tests/backward_cases.py steps its seeds.

A case returns a ``types.SimpleNamespace``; ``*64`` is the fp64 mirror (the reference), ``*32`` the fp32 mirror (the yardstick).
"""
import functools
import math
import types

import numpy as np

from . import rng_reference as rr

SEED_STEPS = 64
F32, F64 = np.float32, np.float64

# ---- edge blocks of box_muller4: printed by tools/find_rng_edges.py, recomputed (not searched) by the tests ------------------------
EDGE_SEED = 0x3DA4F
EDGE_OFFSETS = {"radius_zero": 29601500, "radius_max": 5596761, "angle_zero": 19999506}


def rad32(deg):
    """Degrees -> radians rounded to fp32, as the op layer hands an angle to the entry points."""
    return float(F32(math.radians(deg)))


def _stepped(first, make, ok, what):
    missed = []
    for k in range(SEED_STEPS):
        case = make(first + k)
        why = ok(case)
        if not why:
            case.seed_steps = k
            return case
        missed.append(why)
    raise AssertionError("%s: no seed in %d steps meets the conditions (%s)" % (what, SEED_STEPS, missed[-1]))


def e_ref(a32, a64):
    return float(np.abs(a32.astype(F64) - a64).max())


# ---- base rotations -----------------------------------------------------------------------------------------------------------
POOL_SEED, POOL_SIZE = 0xB0A7, 512


@functools.lru_cache(maxsize=None)
def pool():
    """fp32 Haar rotations (the fp32 mirror's) and the Shepperd branch of each."""
    R = rr.haar_rotation(POOL_SEED, np.arange(POOL_SIZE), F32)
    R.setflags(write=False)
    return R, rr.shepperd_branch(R)


def of_branch(branch, k):
    """The k-th rotation of the pool whose quaternion is extracted by `branch`."""
    R, br = pool()
    return R[np.flatnonzero(br == branch)[k]]


# ---- the Haar stream ----------------------------------------------------------------------------------------------------------
HAAR_MIN_Q = 0.1
# name -> (first seed, offset, N)
HAAR_CASES = {"n4099": (0x5EED0001, 0, 4099),                         # 17 workgroups, a ragged last one
              "high_word": (0x5EED0002, 2 ** 32 - 5, 16),             # the counter's second word changes inside the call
              "offset_2p40": (0x5EED0003, 2 ** 40, 1000),
              "seed_high": (0xC0FFEE1200000005, 12345, 257)}          # key word 1 is not zero
SHARD = ("n4099", 3000, 1099)                                         # rows [3000, 4099) as a call of their own


def _haar(seed, offset, N):
    ctr = [offset + n for n in range(N)]
    q = np.stack(rr.haar_quaternion(seed, ctr, F64), axis=-1)
    c = types.SimpleNamespace(seed=seed, offset=offset, N=N, q_min=float(np.sqrt((q * q).sum(-1)).min()),
                              r64=rr.haar_rotation(seed, ctr, F64), r32=rr.haar_rotation(seed, ctr, F32))
    c.e_ref = e_ref(c.r32, c.r64)
    return c


@functools.lru_cache(maxsize=None)
def haar_case(name):
    seed, offset, N = HAAR_CASES[name]
    return _stepped(seed, lambda s: _haar(s, offset, N), lambda c: "" if c.q_min >= HAAR_MIN_Q else "min |q| %.3f" % c.q_min, name)


@functools.lru_cache(maxsize=None)
def edge_case(kind):
    c = _haar(EDGE_SEED, EDGE_OFFSETS[kind], 1)
    c.words = tuple(int(w[0]) for w in rr.draw(rr.haar_block(EDGE_SEED, [EDGE_OFFSETS[kind]])))
    c.q64 = np.stack(rr.haar_quaternion(EDGE_SEED, [EDGE_OFFSETS[kind]], F64), axis=-1)[0]
    c.q32 = np.stack(rr.haar_quaternion(EDGE_SEED, [EDGE_OFFSETS[kind]], F32), axis=-1)[0]
    return c


# ---- track_advance --------------------------------------------------------------------------------------------------------------
ADVANCE_BATCHES = (1, 257, 65535)                                     # 257: the b += 256 loop takes a second trip
ADVANCE_SEEDS = (0, 1, 2 ** 32, 0x0123456789ABCDEF, 2 ** 64 - 1)
ADVANCE_STEPS = (0, 2 ** 32 - 1, 2 ** 40 + 3)                         # 2^32 - 1: t + 1 carries into the second counter word


# ---- the tracker's predict step ---------------------------------------------------------------------------------------------------
# two workgroups in x, one slot in the second.  The mirror's omega / out cover ALL M slots (a call with n_fresh = 0, so that the
# second workgroup's slot is a noise slot); fresh64 / fresh32 are the last TRACK_FRESH slots of a call with n_fresh = TRACK_FRESH
TRACK_B, TRACK_M, TRACK_N, TRACK_FRESH = 3, 257, 8, 64
TRACK_SIGMA_DEG, TRACK_SIGMA_VEL_DEG, TRACK_DAMPING = 3.0, 1.0, float(F32(0.9))
TRACK_MAX_ANGLE_DEG, TRACK_MAX_SPEED_DEG = 4.6, 3.2                   # about the medians of |omega_p| and |v'|: half the slots clip
CLIP_BAND = 1e-5        # no slot sits this close (relatively) to a clipping decision: fp32 and fp64 decide alike
TRACK_WRAP = 2 ** 48
# name -> (first seed, step, max_angle_deg or None)
DIFFUSE_CASES = {"step_1": (0x7AC4E20000000011, 1, None),
                 "step_2p32": (0x7AC4E20000000011, 2 ** 32 + 1, None),
                 "step_2p47": (0x7AC4E20000000011, 2 ** 47 + 3, None),
                 "clipped": (0x7AC4E20000000021, 2 ** 32 + 1, TRACK_MAX_ANGLE_DEG)}
# name -> (first seed, step, with V, limits)
PREDICT_CASES = {"velocities_limits": (0x7AC4E20000000031, 2 ** 32 + 1, True, True),
                 "no_velocities_limits": (0x7AC4E20000000041, 1, False, True),
                 "velocities_free": (0x7AC4E20000000051, 2 ** 47 + 3, True, False)}


@functools.lru_cache(maxsize=None)
def track_set():
    """R (N,3,3) fp32, two rows per Shepperd branch; idx (B,M) = j mod N with every sample starting at another row; V (B,N,3)."""
    R = np.stack([of_branch(n % 4, n // 4) for n in range(TRACK_N)])
    idx = (np.arange(TRACK_M)[None] + np.arange(TRACK_B)[:, None]) % TRACK_N
    b, n = np.meshgrid(np.arange(TRACK_B), np.arange(TRACK_N), indexing="ij")
    V = (F32(rad32(2.0)) * rr.normals3(rr.diffuse_block(POOL_SEED, 0, b, n), F32)).astype(F32)
    for a in (R, idx, V):
        a.setflags(write=False)
    return R, idx.astype(np.int64), V


def _slots(B=TRACK_B, M=TRACK_M):
    return np.meshgrid(np.arange(B), np.arange(M), indexing="ij")


def _fresh(seed, step, B, M, n_fresh, dtype):
    b, j = _slots(B, M)
    off = rr.tracker_fresh_offset(step, B, b[:, M - n_fresh:], M, j[:, M - n_fresh:])
    return rr.haar_rotation(seed ^ rr.FRESH_XOR, off, dtype)


def _q_min(seed, off):
    q = np.stack(rr.haar_quaternion(seed, off, F64), axis=-1)
    return float(np.sqrt((q * q).sum(-1)).min())


def _fresh_q_min(seed, step, B, M, n_fresh):
    b, j = _slots(B, M)
    return _q_min(seed ^ rr.FRESH_XOR, rr.tracker_fresh_offset(step, B, b[:, M - n_fresh:], M, j[:, M - n_fresh:]))


def _near_band(w64, limit):
    return bool((np.abs(rr.clip_distance(w64, limit)) < CLIP_BAND).any())


def _diffuse(seed, step, max_angle_deg):
    R, idx, _ = track_set()
    B, M, nf = TRACK_B, TRACK_M, TRACK_FRESH
    b, j = _slots()
    sigma, limit = rad32(TRACK_SIGMA_DEG), rad32(max_angle_deg) if max_angle_deg else 0.0
    c = types.SimpleNamespace(seed=seed, step=step, max_angle_deg=max_angle_deg, noise=slice(0, M), fresh=slice(M - nf, M))
    raw64 = F64(sigma) * rr.normals3(rr.diffuse_block(seed, step, b, j), F64)
    raw32 = F32(sigma) * rr.normals3(rr.diffuse_block(seed, step, b, j), F32)
    c.omega64, c.clipped = rr.clip_norm(raw64, limit, F64)
    c.omega32, clipped32 = rr.clip_norm(raw32, limit, F32)
    c.near_band = bool(limit) and _near_band(raw64[:, c.noise], limit)
    c.same_decisions = bool((c.clipped == clipped32)[:, c.noise].all())
    c.out64 = rr.compose_rotation_vector(R[idx], c.omega64, F64)
    c.out32 = rr.compose_rotation_vector(R[idx], c.omega32, F32)
    c.fresh64, c.fresh32 = _fresh(seed, step, B, M, nf, F64), _fresh(seed, step, B, M, nf, F32)
    c.fresh_q_min = _fresh_q_min(seed, step, B, M, nf)
    c.branches = set(rr.shepperd_branch(R[idx][:, c.noise]).reshape(-1).tolist())
    return c


def _two_sided(mask):
    return bool(mask.any() and not mask.all())


def _diffuse_ok(c):
    if c.branches != {0, 1, 2, 3}:
        return "Shepperd branches %s" % sorted(c.branches)
    if c.fresh_q_min < HAAR_MIN_Q:
        return "fresh slots: min |q| %.3f" % c.fresh_q_min
    if c.max_angle_deg and (c.near_band or not c.same_decisions or not _two_sided(c.clipped[:, c.noise])):
        return "clipping: a slot inside the band, or one side of the limit empty"
    return ""


@functools.lru_cache(maxsize=None)
def diffuse_case(name):
    seed, step, limit = DIFFUSE_CASES[name]
    return _stepped(seed, lambda s: _diffuse(s, step, limit), _diffuse_ok, name)


def _predict(seed, step, with_V, limits):
    R, idx, V = track_set()
    B, M, nf = TRACK_B, TRACK_M, TRACK_FRESH
    b, j = _slots()
    sigma, sigma_vel = rad32(TRACK_SIGMA_DEG), rad32(TRACK_SIGMA_VEL_DEG)
    max_angle, max_speed = (rad32(TRACK_MAX_ANGLE_DEG), rad32(TRACK_MAX_SPEED_DEG)) if limits else (0.0, 0.0)
    c = types.SimpleNamespace(seed=seed, step=step, with_V=with_V, limits=limits, noise=slice(0, M), fresh=slice(M - nf, M))
    res = {}
    for dt in (F64, F32):
        v = np.take_along_axis(V, idx[..., None], axis=1).astype(dt) if with_V else np.zeros((B, M, 3), dt)
        y = rr.normals3(rr.velocity_block(seed, step, b, j), dt)
        z = rr.normals3(rr.diffuse_block(seed, step, b, j), dt)
        raw_v = dt(TRACK_DAMPING) * v + dt(sigma_vel) * y
        raw_p = dt(sigma) * z
        vel, clip_v = rr.clip_norm(raw_v, max_speed, dt)
        p, clip_p = rr.clip_norm(raw_p, max_angle, dt)
        omega = vel + p
        out = rr.compose_rotation_vector(R[idx], omega, dt)
        res[dt] = (vel, p, omega, out, clip_v, clip_p, raw_v, raw_p)
    c.vel64, c.p64, c.omega64, c.out64, c.clip_v, c.clip_p, raw_v, raw_p = res[F64]
    c.vel32, c.p32, c.omega32, c.out32 = res[F32][:4]
    c.near_band = limits and (_near_band(raw_v[:, c.noise], max_speed) or _near_band(raw_p[:, c.noise], max_angle))
    c.same_decisions = bool((c.clip_v == res[F32][4])[:, c.noise].all() and (c.clip_p == res[F32][5])[:, c.noise].all())
    c.fresh64, c.fresh32 = _fresh(seed, step, B, M, nf, F64), _fresh(seed, step, B, M, nf, F32)
    c.fresh_q_min = _fresh_q_min(seed, step, B, M, nf)
    c.branches = set(rr.shepperd_branch(R[idx][:, c.noise]).reshape(-1).tolist())
    return c


def _predict_ok(c):
    if c.branches != {0, 1, 2, 3}:
        return "Shepperd branches %s" % sorted(c.branches)
    if c.fresh_q_min < HAAR_MIN_Q:
        return "fresh slots: min |q| %.3f" % c.fresh_q_min
    if c.limits and (c.near_band or not c.same_decisions or not _two_sided(c.clip_v[:, c.noise])
                     or not _two_sided(c.clip_p[:, c.noise])):
        return "clipping: a slot inside the band, or one side of a limit empty"
    return ""


@functools.lru_cache(maxsize=None)
def predict_case(name):
    seed, step, with_V, limits = PREDICT_CASES[name]
    return _stepped(seed, lambda s: _predict(s, step, with_V, limits), _predict_ok, name)


# ---- the pose graph's candidates ---------------------------------------------------------------------------------------------------
GRAPH_B, GRAPH_N, GRAPH_FRESH, GRAPH_SIGMA_DEG = 3, 257, 64, 3.0
GRAPH_SEED = 0x6A4F000900000007
RING16 = tuple((v, (v + 1) % 16) for v in range(16))
# name -> (V, edges (None: the complete graph), k, D): the D = 2 and D = 8 graphs of tests/test_gpu_pose_graph.py at both ends of
# the complete graph's node range, and the ring of 16 of that file's tree test, which alone reaches k = 15
GRAPHS = {"chain3_k1": (3, ((0, 1), (1, 2)), 1, 2), "complete5_k0": (5, None, 0, 8), "complete5_k4": (5, None, 4, 8),
          "ring16_k0": (16, RING16, 0, 2), "ring16_k15": (16, RING16, 15, 2)}
GRAPH_SWEEPS = (0, 255)
GRAPH_TS = (5, 2 ** 32 + 5)
GRAPH_WRAP = 2 ** 40


@functools.lru_cache(maxsize=None)
def graph_rotations(name):
    """A (B,V,3,3) fp32.  A[b][k], the base of the noise slots, takes another Shepperd branch in every sample: three samples
    cannot hold four branches, so graph i leaves out branch (i + 3) mod 4 and the five graphs together hold all four."""
    V, _, k, _ = GRAPHS[name]
    i = sorted(GRAPHS).index(name)
    R, _ = pool()
    A = np.array(R[64 + 48 * i:64 + 48 * i + GRAPH_B * V].reshape(GRAPH_B, V, 3, 3))
    for b in range(GRAPH_B):
        A[b, k] = of_branch((i + b) % 4, 8 + i)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def graph_case(name, sweep, t):
    V, _, k, D = GRAPHS[name]
    B, N, nf = GRAPH_B, GRAPH_N, GRAPH_FRESH
    A = graph_rotations(name)
    sigma = rad32(GRAPH_SIGMA_DEG)
    c = types.SimpleNamespace(seed=GRAPH_SEED, sweep=sweep, t=t, k=k, D=D, V=V, A=A, noise=slice(1 + D, N - nf), fresh=slice(N - nf, N))
    b, n = np.meshgrid(np.arange(B), np.arange(N)[c.noise], indexing="ij")
    base = np.broadcast_to(A[:, k][:, None], n.shape + (3, 3))
    c.q64 = rr.compose_rotation_vector(base, F64(sigma) * rr.normals3(rr.graph_block(c.seed, t, sweep, b, k, n), F64), F64)
    c.q32 = rr.compose_rotation_vector(base, F32(sigma) * rr.normals3(rr.graph_block(c.seed, t, sweep, b, k, n), F32), F32)
    b, n = np.meshgrid(np.arange(B), np.arange(N)[c.fresh], indexing="ij")
    off = rr.graph_fresh_offset(t, sweep, b, k, N, n)
    c.fresh64, c.fresh32 = rr.haar_rotation(c.seed ^ rr.FRESH_XOR, off, F64), rr.haar_rotation(c.seed ^ rr.FRESH_XOR, off, F32)
    c.fresh_q_min = _q_min(c.seed ^ rr.FRESH_XOR, off)
    c.branches = set(rr.shepperd_branch(A[:, k]).tolist())
    return c
