"""CPU model of the dV scatter's lane map (3dahv_amd/csrc/ahv_bwd_volume.hip, kernel 2b): the plain read-modify-write of
score_backward_volume_rmw_kernel is a data race unless the 8 voxels of one scatter instruction have disjoint LIVE
footprints for every matrix rmw_rotation_like accepts.  The acceptance threshold is read out of the source, so loosening
it fails here, on the CPU, without touching this file.

What the model mirrors:
  * sample coordinate i = R (idx - 3.5) + 3.5 per axis, x fastest -- gather_lane / gather_hyp / gather_coord of
    csrc/ahv_dual.h (rows 0, 1, 2 of R give x, y, z; columns multiply x, y, z);
  * base row clamp(floor(i), 0, 6) and hat weights max(0, 1 - |i - row|) of rows base, base + 1 -- hat_axis of ahv_dual.h;
  * a corner whose weight product is exactly 0 goes to the trash row -- ``off[n] = (w[n] != 0.0f) ? o : kImgTrashBytes`` in
    rmw_corners; so a row of an axis is live when its hat weight is non-zero.  The model calls it live from -1e-5 on: a
    superset that absorbs the kernel's fp32 coordinate chain (|i| < 16, three fmas: < 1e-5);
  * a step is the 8 voxels (z0 + 4 a, y0 + 4 b, x0 + 4 c), z0, y0, x0 in 0..3 -- rmw_scatter_half: lane = (ab, vx, corner),
    ``xl = xbuf + 2 * ab * kXPlane + 4 * (vx >> 1) * kXRow + 16 * (vx & 1)`` and the matching ``trow``, with the step
    S = (ap, b0, e0) of rmw_step_load added on top: depth 2 H + ap + 4 ab (rmw_dx_half: plane al holds depth
    2 H + (al & 1) + 4 (al >> 1), and al = ap + 2 ab), y = b0 + 4 (vx >> 1), x = e0 + 4 (vx & 1).
Two voxels collide when they share a live row on all three axes (a footprint is the product of its axes' live rows)."""
import os
import re

import numpy as np

from . import rotation_families as fam
from .conftest import REPO

LIVE_EPS = 1e-5


def _source():
    return open(os.path.join(REPO, "3dahv_amd", "csrc", "ahv_bwd_volume.hip")).read()


def parsed_threshold():
    body = re.search(r"bool rmw_rotation_like\(const float\* Rm\)\s*\{(.*?)\n\}", _source(), flags=re.S).group(1)
    found = re.findall(r"fabsf\(d\)\s*<=\s*([0-9.eE+-]+)f", body)
    assert len(found) == 1, found
    return float(found[0])


def classifier_fp32(R, thr):
    """rmw_rotation_like restated: the same fmaf chain per entry of R^T R (an fma = exact product and sum in fp64, rounded
    to fp32 once), compared in fp32.  R (n,3,3) fp32, row-major like the kernel's Rm[9]."""
    Rm = np.asarray(R, dtype=np.float32).reshape(-1, 9).astype(np.float64)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    ok = np.ones(Rm.shape[0], dtype=bool)
    for i in range(3):
        for j in range(i, 3):
            d = f32(f32(Rm[:, i] * Rm[:, j] + f32(Rm[:, 3 + i] * Rm[:, 3 + j] + f32(Rm[:, 6 + i] * Rm[:, 6 + j]))) - (1.0 if i == j else 0.0))
            ok &= np.abs(d).astype(np.float32) <= np.float32(thr)
    return ok


def live_masks(R):
    """(n, 512, 3) bit masks of the live rows (bit r = row r) of every voxel (index z * 64 + y * 8 + x) on axes x, y, z."""
    R = np.asarray(R, dtype=np.float32).astype(np.float64)
    c = np.arange(8) - 3.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    P = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=-1)              # (512, 3): columns of R multiply (x, y, z)
    i = np.einsum("nab,pb->npa", R, P) + 3.5
    base = np.clip(np.floor(i), 0, 6)
    live0 = (1.0 - np.abs(i - base)) > -LIVE_EPS
    live1 = (1.0 - np.abs(i - base - 1.0)) > -LIVE_EPS
    b = base.astype(np.int64)
    return (live0.astype(np.int64) << b) | (live1.astype(np.int64) << (b + 1))


def overlapping_pairs(R):
    """(n,) number of voxel pairs, summed over the 64 steps, that share a live row."""
    m = live_masks(R)
    n = m.shape[0]
    m = m.reshape(n, 2, 4, 2, 4, 2, 4, 3).transpose(0, 2, 4, 6, 1, 3, 5, 7).reshape(n, 64, 8, 3)   # (n, step (z0,y0,x0), voxel (a,b,c), axis)
    hit = ((m[:, :, :, None, :] & m[:, :, None, :, :]) != 0).all(axis=-1)
    hit &= ~np.eye(8, dtype=bool)
    return hit.sum(axis=(1, 2, 3)) // 2


def rotation_onto(a, b):
    """The rotation about a x b that takes unit vector a to unit vector b (a != -b)."""
    v, c = np.cross(a, b), float(a @ b)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + k + k @ k / (1.0 + c)


def test_the_model_knows_an_overlap_when_it_sees_one():
    """Known answers: identity and a cube rotation keep the 8 voxels of a step 4 rows apart; the zero matrix puts all 512
    samples on (3.5, 3.5, 3.5): every one of the 28 pairs of every step collides; 0.25 I maps voxels 4 apart one row apart."""
    cube = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    R = np.stack([np.eye(3, dtype=np.float32), cube, np.zeros((3, 3), np.float32), 0.25 * np.eye(3, dtype=np.float32)])
    assert overlapping_pairs(R).tolist() == [0, 0, 64 * 28, 64 * 28]
    m = live_masks(np.eye(3, dtype=np.float32)[None])[0]
    assert m[0].tolist() == [0b11, 0b11, 0b11] and m[511].tolist() == [0b11000000] * 3   # integer samples: both rows count as live


def test_accepted_matrices_have_disjoint_footprints_in_every_step():
    R, names = fam.inside()
    bad = overlapping_pairs(R)
    assert not bad.any(), [names[k] for k in np.nonzero(bad)[0]]
    assert not overlapping_pairs(fam.haar(np.random.RandomState(11), 200)).any()


def test_every_matrix_up_to_the_kernels_threshold_has_disjoint_footprints():
    """Matrices Q (I + E)^(1/2) (R^T R = I + E exactly) around Haar rotations: 256 with the six free entries of E uniform
    in +-threshold, and all 64 sign patterns of E at 0.999 x threshold on each of three rotations.  A draw is rejected unless
    I + E is positive definite and the fp32 classifier, run with the PARSED threshold, accepts the fp32 matrix -- so these
    are exactly matrices the shipped kernel scatters in parallel.  A third group aims: the extreme E again, with Q turning
    the image of one of the 13 lattice directions onto the cube diagonal, where its length is spread evenly over the axes.
    (Where the limit is: two voxels can only share a row on all three axes if |R v|^2 < 12 for their difference v = 4 (a, b, c),
    a, b, c in {-1, 0, 1}; |R v|^2 = 16 v^T (I + E) v >= 16 (k - k^2 d) for k non-zero entries and entrywise deviation d, so
    nothing collides up to d = 0.25.  The kernel's comment argues through the eigenvalues of R^T R, which is valid and more
    conservative.  With the constant at 0.3 this test finds colliding matrices in the second and third group.)"""
    thr = parsed_threshold()
    assert 0.0 < thr < 1.0
    rs = np.random.RandomState(13)
    iu = np.triu_indices(3)
    out = []

    def take(q, vals):
        e = np.zeros((3, 3))
        e[iu] = vals
        e = e + e.T - np.diag(np.diag(e))
        if np.linalg.eigvalsh(np.eye(3) + e).min() <= 1e-3:
            return False
        r = (q @ fam.sqrt_spd(np.eye(3) + e)).astype(np.float32)
        if not classifier_fp32(r[None], thr)[0]:
            return False
        out.append(r)
        return True
    tries = 0
    while len(out) < 256:
        tries += 1
        assert tries < 20000, "rejection sampling does not terminate"
        take(fam.haar(rs, 1)[0], rs.uniform(-thr, thr, 6))
    extreme = 0
    for q in fam.haar(rs, 3):
        for bits in range(64):
            extreme += take(q, [0.999 * thr * (1 if (bits >> k) & 1 else -1) for k in range(6)])
    assert extreme >= 96    # (sign patterns that leave I + E indefinite only exist for a threshold >= 1/3)
    # aimed: the same extreme E with Q chosen so that the image of a lattice difference v lies on the cube diagonal
    diag = np.ones(3) / np.sqrt(3.0)
    dirs = [np.array(v, dtype=np.float64) for v in np.ndindex(3, 3, 3) if v > (1, 1, 1)]     # 13 directions of {-1, 0, 1}^3 up to sign
    for bits in range(64):
        vals = [0.999 * thr * (1 if (bits >> k) & 1 else -1) for k in range(6)]
        e = np.zeros((3, 3))
        e[iu] = vals
        e = e + e.T - np.diag(np.diag(e))
        if np.linalg.eigvalsh(np.eye(3) + e).min() <= 1e-3:
            continue
        s = fam.sqrt_spd(np.eye(3) + e)
        for v in dirs:
            w = s @ (v - 1.0)
            take(rotation_onto(w / np.linalg.norm(w), diag), vals)
    R = np.stack(out)
    dev = fam.deviation(R)
    assert dev.max() <= thr * (1 + 1e-5) and dev.max() > 0.99 * thr and (dev > 0.5 * thr).mean() > 0.5
    bad = overlapping_pairs(R)
    assert not bad.any(), "%d of %d accepted matrices (threshold %g) have voxels of one step sharing a live row, e.g. deviation %.4f" % (
        int((bad > 0).sum()), len(R), thr, float(dev[bad > 0].min()))


def test_the_classifier_separates_the_families_in_fp32():
    thr = parsed_threshold()
    Ri, ni = fam.inside()
    Ro, no = fam.outside()
    assert classifier_fp32(Ri, thr).all() and not classifier_fp32(Ro, thr).any()
    # ... and agrees with fp64: every matrix keeps its distance from the threshold
    assert fam.deviation(Ri).max() <= thr - fam.MARGIN and fam.deviation(Ro).min() >= thr + fam.MARGIN
    assert len(set(ni)) == len(ni) and len(set(no)) == len(no) and no[-1].startswith("zero")
    for kinds, names in ((fam.INSIDE, ni), (fam.OUTSIDE, no)):
        assert {fam.family(s) for s in names} >= set(kinds)
    assert np.linalg.svd(Ro.astype(np.float64), compute_uv=False).max() < 1.8
    assert fam.inside()[0].tobytes() == Ri.tobytes() and Ri.dtype == np.float32 and Ri.shape == (len(ni), 3, 3)


def test_rejected_matrices_do_overlap():
    """A condition on the fixtures: at least a quarter of ``outside`` collides under the model, otherwise the GPU tests that
    use it would not exercise what the one-voxel-per-instruction path exists for."""
    R, names = fam.outside()
    share = (overlapping_pairs(R) > 0).mean()
    assert share >= 0.25, share


def test_mixed_keeps_both_kinds_in_a_workgroup_for_any_grid():
    """The two slots of a workgroup hold hypotheses h and h + gridDim.x: for every grid width that can occur (1..256, and
    wider) a good share of those pairs is one accepted and one rejected matrix, and the other combinations occur too."""
    for n in (200, 2000):
        R, names, is_in = fam.mixed(n)
        thr = parsed_threshold()
        assert np.array_equal(classifier_fp32(R, thr), is_in) and is_in.sum() == n // 2
        assert [fam.family(s) in fam.INSIDE for s in names] == is_in.tolist()
        for g in range(1, min(n // 2, 304) + 1):
            a, b = is_in[:-g], is_in[g:]
            assert (a != b).mean() >= 0.3 and (a & b).any() and (~a & ~b).any(), (n, g)
