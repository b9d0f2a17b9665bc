"""Matrix families for the dV scatter of the backward (3dahv_amd/csrc/ahv_bwd_volume.hip, score_backward_volume_rmw_kernel).

The kernel classifies every hypothesis with rmw_rotation_like -- max |R^T R - I| <= 0.04 entrywise -- and scatters the
8 voxels of a step in ONE instruction when the matrix passes, one voxel per instruction otherwise.  ``inside`` holds
matrices the classifier accepts, pushed towards the threshold; ``outside`` matrices it must reject, from just behind
the threshold to rank-deficient ones; ``mixed`` both.  Plain module (like tests/procfill.py), deterministic
(``np.random.RandomState``: legacy MT19937 stream, bit-stable across numpy versions), built in fp64 and returned as
fp32 arrays with one name per matrix.  Every matrix keeps max |R^T R - I| at least 1e-3 away from 0.04, so the fp32
classifier of the kernel and an fp64 evaluation agree about it; no matrix scales by 1.8 or more (whole positions
would fall outside the volume; ``double`` of the edge_rotations fixture covers that).

Sub-families, dealt round-robin (matrix k belongs to sub-family k mod the number of sub-families):
  inside   scale_lo / scale_hi   s Q, s^2 = 0.962 / 1.038                              deviation 0.038 (diagonal)
           sym                   Q (I + E)^(1/2), E symmetric, all six free entries +-0.038   deviation 0.038 (all entries)
           reflect               Haar rotation with one column negated (det = -1)      deviation ~1e-7
           rot                   Haar rotation                                         deviation ~1e-7
  outside  scale_045lo / _045hi  s Q, s^2 = 0.955 / 1.045                              deviation 0.045
           sym045                Q (I + E)^(1/2), ONE off-diagonal pair of E = +-0.045 deviation 0.045
           shrink                s Q, s uniform in [0.5, 0.8]                          deviation 0.36 .. 0.75
           proj110               Q diag(1, 1, 0)                                       rank 2
           proj1p30              Q diag(1, 0.3, 0)                                     rank 2, one direction squeezed
           proj100               Q diag(1, 0, 0)                                       rank 1
           shear                 Q (I + 0.6 e0 e1^T)
           zero                  the zero matrix (once, the last matrix of the family)
Measured with the CPU model of tests/test_rmw_footprints_cpu.py (seed 7): ``inside(96)`` max deviation 0.0380, no
matrix with overlapping footprints; ``outside(168)`` 78 of 168 matrices (46 %) with voxels of one scatter step sharing a
live row: shrink 14 of 21, proj110 / proj1p30 / proj100 21 of 21 each, zero; none of scale_045lo / scale_045hi / sym045
/ shear (they are behind the classifier's threshold but far from the geometric limit, an entrywise deviation of 0.25);
200 Haar rotations: none; ``mixed(200)`` 42, ``mixed(2000)`` 432 matrices with overlaps.
"""
import numpy as np

THRESHOLD_DOC = 0.04          # what the families are laid out around (the test parses the kernel's own constant)
MARGIN = 1e-3                 # every matrix stays this far from THRESHOLD_DOC in max |R^T R - I|
INSIDE = ("scale_lo", "scale_hi", "sym", "reflect", "rot")
OUTSIDE = ("scale_045lo", "scale_045hi", "sym045", "shrink", "proj110", "proj1p30", "proj100", "shear")
RANK_DEFICIENT = ("proj110", "proj1p30", "proj100", "zero")


def haar(rs, n):
    """n Haar rotations (fp64, det = +1) from ``rs``: QR of a Gaussian matrix with the signs of R's diagonal fixed."""
    a = rs.standard_normal((n, 3, 3))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return q


def sqrt_spd(m):
    w, v = np.linalg.eigh(m)
    assert w.min() > 0
    return (v * np.sqrt(w)) @ v.T


def deviation(R):
    """max |R^T R - I| entrywise per matrix, in fp64."""
    R = np.asarray(R, dtype=np.float64)
    return np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).reshape(R.shape[:-2] + (9,)).max(axis=-1)


def family(name):
    return name.rsplit("_", 1)[0]


def is_full_rank(name):
    return family(name) not in RANK_DEFICIENT


def _one(kind, q, rs):
    eye = np.eye(3)
    if kind in ("scale_lo", "scale_hi", "scale_045lo", "scale_045hi"):
        return np.sqrt({"scale_lo": 0.962, "scale_hi": 1.038, "scale_045lo": 0.955, "scale_045hi": 1.045}[kind]) * q
    if kind == "sym":
        e = np.zeros((3, 3))
        for i in range(3):
            for j in range(i, 3):
                e[i, j] = e[j, i] = 0.038 * (1 if rs.randint(2) else -1)
        return q @ sqrt_spd(eye + e)
    if kind == "sym045":
        i, j = [(0, 1), (0, 2), (1, 2)][rs.randint(3)]
        e = np.zeros((3, 3))
        e[i, j] = e[j, i] = 0.045 * (1 if rs.randint(2) else -1)
        return q @ sqrt_spd(eye + e)
    if kind == "reflect":
        r = q.copy()
        r[:, rs.randint(3)] *= -1
        return r
    if kind == "rot":
        return q
    if kind == "shrink":
        return rs.uniform(0.5, 0.8) * q
    if kind == "proj110":
        return q @ np.diag([1.0, 1.0, 0.0])
    if kind == "proj1p30":
        return q @ np.diag([1.0, 0.3, 0.0])
    if kind == "proj100":
        return q @ np.diag([1.0, 0.0, 0.0])
    if kind == "shear":
        s = eye.copy()
        s[0, 1] = 0.6
        return q @ s
    raise KeyError(kind)


def _build(kinds, n, seed, zero_last):
    rs = np.random.RandomState(seed)
    q = haar(rs, n)
    R = np.empty((n, 3, 3))
    names = []
    for k in range(n):
        kind = kinds[k % len(kinds)]
        R[k] = _one(kind, q[k], rs)
        names.append("%s_%d" % (kind, k))
    if zero_last and n:
        R[-1] = 0.0
        names[-1] = "zero_%d" % (n - 1)
    return np.ascontiguousarray(R.astype(np.float32)), names


def inside(n=96, seed=7):
    """(R (n,3,3) fp32, names): matrices rmw_rotation_like accepts; max |R^T R - I| <= 0.04 - MARGIN."""
    R, names = _build(INSIDE, n, seed, False)
    assert n == 0 or deviation(R).max() <= THRESHOLD_DOC - MARGIN
    return R, names


def outside(n=168, seed=7):
    """(R (n,3,3) fp32, names): matrices rmw_rotation_like must reject; max |R^T R - I| >= 0.04 + MARGIN, all singular
    values below 1.8.  The last one is the zero matrix."""
    R, names = _build(OUTSIDE, n, seed + 1000, True)
    assert n == 0 or (deviation(R).min() >= THRESHOLD_DOC + MARGIN and np.linalg.svd(R.astype(np.float64), compute_uv=False).max() < 1.8)
    return R, names


def mixed(n=200, seed=7):
    """(R, names, is_inside (n,) bool): inside(n // 2) and outside(n - n // 2) interleaved in a fixed pseudo-random order.
    The two slots of a workgroup of the dV kernel work on hypotheses h and h + gridDim.x at the same time, and gridDim.x
    depends on the device and on B: a strict alternation would put the same kind into both slots whenever it is even.  In
    this order about half of the pairs (h, h + g) hold one matrix of each kind for EVERY g (the model test checks every width up to 304),
    the others two accepted or two rejected ones."""
    ri, ni = inside(n // 2, seed)
    ro, no = outside(n - n // 2, seed)
    is_in = np.zeros(n, dtype=bool)
    is_in[np.random.RandomState(seed + 2000).permutation(n)[:n // 2]] = True
    R = np.empty((n, 3, 3), dtype=np.float32)
    R[is_in], R[~is_in] = ri, ro
    it_i, it_o = iter(ni), iter(no)
    names = [next(it_i) if f else next(it_o) for f in is_in]
    return R, names, is_in
