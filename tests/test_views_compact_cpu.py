"""Angle-limited multi-view verification, compact -- CPU tier: argument validation of ``ahv_view_rotations_compact_f32`` /
``ahv_fuse_view_scores_compact_f32`` through the ctypes table (validation runs before any HIP call), what the op layer refuses,
hand cases of the numpy reference (tests/views_compact_reference.py) and ``ops.haar_view_fraction`` against Haar samples."""
import ctypes
import math

import numpy as np
import pytest
import torch

from . import views_compact_reference as vcr
from . import views_reference as vr


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def W(*v):
    return (ctypes.c_float * len(v))(*v)


def caller(fn, ok):
    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return call


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------

def test_view_rotations_compact_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    tau = float(vr.tau_of(60.0))
    need = lib.ahv_view_rotations_compact_workspace_bytes
    assert need(1, 3, 10) == 4 * 3 and need(2, 3, 1024) == 4 * 6 and need(2, 3, 1025) == 4 * 12 and need(1, 16, 50000) == 4 * 16 * 49
    assert need(0, 3, 10) == need(1, 0, 10) == need(1, 17, 10) == need(1, 3, 0) == 0
    # (Q, q_batch_stride, A, weights, B, V, N, min_trace, capacity, out, slot, counts, workspace, workspace_bytes, stream)
    call = caller(lib.ahv_view_rotations_compact_f32, [1, 0, 1, None, 1, 3, 10, tau, 4, 1, 1, 1, 16, 12, None])
    for bad in (0, 17, -1):
        assert call(_5=bad) == -1 and b"V = " in err() and str(bad).encode() in err()
    for kw in ({"_4": 0}, {"_4": -1}, {"_6": 0}, {"_6": -3}):
        assert call(**kw) == -1 and b"at least 1" in err()
    assert call(_4=65536) == -1 and b"65535" in err()
    for bad in (0, 11, -1):
        assert call(_8=bad) == -1 and b"capacity" in err() and b"1..N" in err(), bad
    assert call(_6=1 << 31, _8=4) == -1 and b"2^31" in err()
    assert call(_6=(1 << 31) + 5, _8=4) == -1 and b"2^31" in err()
    for bad in (5, 89, 91, -90):
        assert call(_1=bad) == -1 and b"q_batch_stride" in err()
    for bad in (-1.0, 3.0, float("nan"), float("inf"), -float("inf"), 3.5, -1.5):
        assert call(_7=bad) == -1 and b"min_trace" in err(), bad
    for at in (0, 2, 11):                                      # Q, A, counts
        assert call(**{"_%d" % at: None}) == -1 and b"null" in err(), at
    assert call(_9=None) == -1 and b"out and slot" in err()    # one without the other ...
    assert call(_10=None) == -1 and b"out and slot" in err()
    for bad in (W(1.0, -0.5, 1.0), W(1.0, float("nan"), 1.0), W(float("inf"), 1.0, 1.0)):
        assert call(_3=bad) == -1 and b"weights[" in err() and b"finite" in err()
    assert call(_3=W(0.0, -0.0, 0.0)) == -1 and b"all zero" in err()
    assert call(_13=11) == -1 and b"workspace of 12 bytes" in err() and b"got 11" in err()
    assert call(_12=None) == -1 and b"workspace" in err()
    assert call(_12=18) == -1 and b"aligned" in err()
    assert call(_9=None, _10=None, _13=8) == -1 and b"workspace" in err()   # ... and the count-only call is checked alike
    L = ahv._lib
    assert (L.AHV_VIEW_SLOT_EXCLUDED, L.AHV_VIEW_SLOT_OVERFLOW) == (-1, -2) == (vcr.EXCLUDED, vcr.OVERFLOW)
    assert lib.ahv_abi_version() == (2 << 16) | 3             # added under 2.3: callers probe for the symbol


def test_fuse_view_scores_compact_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    # (scores, slot, weights, B, V, N, capacity, n_offset, fused, best_key, flags, stream)
    call = caller(lib.ahv_fuse_view_scores_compact_f32, [1, 1, None, 1, 3, 10, 4, 0, 1, 1, 0, None])
    for bad in (0, 17, -1):
        assert call(_4=bad) == -1 and b"V = " in err() and str(bad).encode() in err()
    for kw in ({"_3": 0}, {"_5": 0}, {"_5": -3}):
        assert call(**kw) == -1 and b"at least 1" in err()
    assert call(_3=65536) == -1 and b"65535" in err()
    for bad in (0, 11, -1):
        assert call(_6=bad) == -1 and b"capacity" in err() and b"1..N" in err(), bad
    assert call(_5=1 << 31) == -1 and b"2^31" in err()
    assert call(_7=1 << 32) == -1 and b"32 bits" in err()
    assert call(_7=-1) == -1 and b"32 bits" in err()
    for bad in (2, 3, 4, 128):                                 # AHV_VIEWS_NO_ANGLE_LIMIT has no meaning here
        assert call(_10=bad) == -1 and b"flags" in err(), bad
    for at in (0, 1, 9):                                       # scores, slot, best_key
        assert call(**{"_%d" % at: None}) == -1 and b"null" in err(), at
    for bad in (W(1.0, -0.5, 1.0), W(1.0, float("nan"), 1.0), W(float("inf"), 1.0, 1.0)):
        assert call(_2=bad) == -1 and b"weights[" in err() and b"finite" in err()
    assert call(_2=W(0.0, 0.0, 0.0)) == -1 and b"all zero" in err()
    assert lib.ahv_abi_version() == (2 << 16) | 3


# ---- the op layer without a GPU -------------------------------------------------------------------------------

def test_compact_ops_refuse_cpu_tensors_bad_arguments_and_autograd(ahv):
    ops = ahv.ops
    Q = torch.eye(3)[None].repeat(8, 1, 1)
    A = torch.eye(3)[None, None].repeat(2, 3, 1, 1)
    s, slot = torch.zeros(2, 3, 4), torch.zeros(2, 3, 8, dtype=torch.int32)
    vols = (torch.zeros(2, 3, 16, 8, 8, 8), torch.zeros(2, 16, 8, 8, 8))
    head = (torch.zeros(32, 384), torch.zeros(32, 32), torch.zeros(32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_rotations_compact(Q, A, 60.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fuse_view_scores_compact(s, slot)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.verify_views(*vols, Q, A, *head, max_view_angle_deg=60.0, compact=True)
    with pytest.raises(RuntimeError, match="max_view_angle_deg"):
        ops.verify_views(*vols, Q, A, *head, compact=True)
    with pytest.raises(RuntimeError, match="max_view_angle_deg"):
        ops.view_rotations_compact(Q, A, None)
    with pytest.raises(RuntimeError, match="compact=True"):
        ops.verify_views(*vols, Q, A, *head, max_view_angle_deg=60.0, capacity=4)
    with pytest.raises(RuntimeError, match="compact=True"):
        ops.verify_views(*vols, Q, A, *head, want_counts=True)
    for bad in (0, 9, -1):
        with pytest.raises(RuntimeError, match="capacity"):
            ops.view_rotations_compact(Q, A, 60.0, capacity=bad)
        with pytest.raises(RuntimeError, match="capacity"):
            ops.verify_views(*vols, Q, A, *head, max_view_angle_deg=60.0, compact=True, capacity=bad)
    with pytest.raises(RuntimeError, match="capacity"):
        ops.fuse_view_scores_compact(torch.zeros(2, 3, 9), slot)
    for bad in (0.0, 180.0, float("nan")):
        with pytest.raises(RuntimeError, match="min_angle_deg"):
            ops.view_rotations_compact(Q, A, bad)
    with pytest.raises(RuntimeError, match="V = 17"):
        ops.view_rotations_compact(Q, torch.eye(3)[None, None].repeat(2, 17, 1, 1), 60.0)
    with pytest.raises(RuntimeError, match="V = 17"):
        ops.fuse_view_scores_compact(torch.zeros(2, 17, 4), torch.zeros(2, 17, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="Q must be"):
        ops.view_rotations_compact(torch.eye(3)[None, None].repeat(3, 8, 1, 1), A, 60.0)
    with pytest.raises(RuntimeError, match="A must be"):
        ops.view_rotations_compact(Q, A[0], 60.0)
    with pytest.raises(RuntimeError, match=r"\(B,V,M\)"):
        ops.fuse_view_scores_compact(s, slot[:1])
    with pytest.raises(RuntimeError, match="weights must hold"):
        ops.view_rotations_compact(Q, A, 60.0, weights=[1.0, 1.0])
    with pytest.raises(RuntimeError, match="weights must hold"):
        ops.fuse_view_scores_compact(s, slot, weights=[1.0, 1.0])
    with pytest.raises(RuntimeError, match="vol_refs"):
        ops.verify_views(torch.zeros(2, 2, 16, 8, 8, 8), vols[1], Q, A, *head, max_view_angle_deg=60.0, compact=True)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.view_rotations_compact(Q.clone().requires_grad_(True), A, 60.0)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.fuse_view_scores_compact(s.clone().requires_grad_(True), slot)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.verify_views(vols[0].clone().requires_grad_(True), vols[1], Q, A, *head, max_view_angle_deg=60.0, compact=True)


def test_aligner_verify_views_forwards_the_compact_keywords(ahv):
    fa = ahv.aligner.Feature_Aligner(in_channel=64, mid_channel=32, out_channel=32, n_heads=4, depth=1).eval()
    Q = torch.eye(3)[None].repeat(8, 1, 1)
    A = torch.eye(3)[None, None].repeat(1, 2, 1, 1)
    refs, query = torch.zeros(1, 2, 16, 8, 8, 8), torch.zeros(1, 16, 8, 8, 8)
    with pytest.raises(RuntimeError, match="max_view_angle_deg"):
        fa.verify_views(refs, query, Q, A, compact=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.verify_views(refs, query, Q, A, compact=True, max_view_angle_deg=90.0)


# ---- hand cases of the reference ------------------------------------------------------------------------------

def _haar(ahv, n, seed):
    return ahv.rotations.haar_rotations_np(n, seed=seed)


def _angle_to_identity(Q):
    return np.degrees(np.arccos(np.clip((np.trace(Q.astype(np.float64), axis1=1, axis2=2) - 1) / 2, -1, 1)))


def test_all_excluded_gives_zero_counts_and_every_slot_minus_one(ahv):
    Q = _haar(ahv, 64, 7)
    A = np.broadcast_to(np.eye(3, dtype=np.float32), (1, 2, 3, 3))
    theta = float(_angle_to_identity(Q).min()) * 0.5
    slot, counts, g, margin = vcr.compact(Q, A, theta)
    assert not g.any() and margin > 0 and counts.tolist() == [[0, 0]] and np.all(slot == vcr.EXCLUDED)
    R = vcr.gather(vr.view_rotations(Q, A), slot, 1)             # M = max(1, 0): one identity per view
    assert R.shape == (1, 2, 1, 3, 3) and np.array_equal(R[0, :, 0], np.broadcast_to(np.eye(3), (2, 3, 3)))


def test_slots_number_the_participating_hypotheses_in_order(ahv):
    Q = _haar(ahv, 300, 11)
    A = np.broadcast_to(np.eye(3, dtype=np.float32), (1, 1, 3, 3))
    ang = _angle_to_identity(Q)
    theta = float(np.median(ang))
    slot, counts, g, _ = vcr.compact(Q, A, theta)
    inside = np.flatnonzero(ang <= theta)
    assert counts.tolist() == [[inside.size]] and 0 < inside.size < 300
    assert slot[0, 0, inside].tolist() == list(range(inside.size)) and np.all(np.delete(slot[0, 0], inside) == vcr.EXCLUDED)
    R = vr.view_rotations(Q, A)
    assert np.array_equal(vcr.gather(R, slot, inside.size)[0, 0], R[0, 0, inside])
    s = np.arange(inside.size, dtype=np.float32)[None, None]
    full = vcr.scatter(s, slot)
    assert np.array_equal(full[0, 0, inside], s[0, 0]) and np.isnan(np.delete(full[0, 0], inside)).all()


def test_a_nan_entry_in_a_hypothesis_takes_it_out(ahv):
    Q = _haar(ahv, 16, 9)
    Q[:] = Q[0]                                       # every hypothesis sits on view 0's pose
    A = Q[:1].reshape(1, 1, 3, 3).copy()
    Q[5, 1, 2] = np.nan
    slot, counts, g, _ = vcr.compact(Q, A, 60.0)
    assert counts.tolist() == [[15]] and slot[0, 0, 5] == vcr.EXCLUDED
    assert np.delete(slot[0, 0], 5).tolist() == list(range(15))


def test_a_zero_weight_view_has_count_zero(ahv):
    Q, A = _haar(ahv, 50, 3), _haar(ahv, 6, 4).reshape(2, 3, 3, 3)
    slot, counts, g, _ = vcr.compact(Q, A, 150.0, [1.0, 0.0, 3.0])
    assert counts[:, 1].tolist() == [0, 0] and np.all(slot[:, 1] == vcr.EXCLUDED)
    assert (counts[:, 0] > 0).all() and (counts[:, 2] > 0).all()
    full, _, _, _ = vcr.compact(Q, A, 150.0)          # the same view with a weight takes part
    assert (full[:, 1] >= 0).any() and np.array_equal(full[:, 0], slot[:, 0])


def test_overflow_marks_exactly_the_last_participating_hypotheses(ahv):
    Q, A = _haar(ahv, 400, 21), _haar(ahv, 2, 22).reshape(1, 2, 3, 3)
    slot, counts, g, _ = vcr.compact(Q, A, 120.0)
    cap = int(counts.min()) - 1
    assert cap >= 2
    cut, counts_cut, _, _ = vcr.compact(Q, A, 120.0, capacity=cap)
    assert np.array_equal(counts_cut, counts)                    # never clipped
    for v in range(2):
        n_in = np.flatnonzero(g[0, v])
        assert np.array_equal(np.flatnonzero(cut[0, v] == vcr.OVERFLOW), n_in[cap:]) and n_in[cap:].size == counts[0, v] - cap
        assert cut[0, v, n_in[:cap]].tolist() == list(range(cap))
        assert np.array_equal(cut[0, v] == vcr.EXCLUDED, ~g[0, v])


# ---- the Haar share ------------------------------------------------------------------------------------------

def test_haar_view_fraction_formula_and_samples(ahv):
    f = ahv.ops.haar_view_fraction
    assert abs(f(90) - (math.pi / 2 - 1) / math.pi) <= 1e-12
    assert f(0) == 0.0 and abs(f(180) - 1.0) <= 1e-12 and abs(f(60) - 0.0577) < 1e-3 and abs(f(150) - 0.674) < 1e-3
    for bad in (-1.0, 181.0, float("nan")):
        with pytest.raises(RuntimeError, match="max_view_angle_deg"):
            f(bad)
    n = 200000
    Q = _haar(ahv, n, 31)
    fixed = _haar(ahv, 1, 32)[0].astype(np.float64)
    t = np.einsum("nij,ij->n", Q.astype(np.float64), fixed)      # trace of the relative rotation to a fixed one
    for theta in (60.0, 90.0):
        p = f(theta)
        share = float(np.mean(t >= 1.0 + 2.0 * math.cos(math.radians(theta))))
        sigma = math.sqrt(p * (1.0 - p) / n)
        print("theta %g: formula %.5f, sample %.5f, %.2f sigma" % (theta, p, share, (share - p) / sigma))
        assert abs(share - p) <= 5.0 * sigma
