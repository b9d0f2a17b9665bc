"""Multi-view verification, CPU tier: argument validation of ``ahv_view_rotations_f32`` / ``ahv_fuse_view_scores_f32`` through
the ctypes table (validation runs before any HIP call), the numpy reference (tests/views_reference.py) against the fixture the
reference's own code produced (G13 ``multiview``, tools/gen_golden.py gen_multiview), and hand cases of the reference."""
import ctypes

import numpy as np
import pytest
import torch

from . import views_reference as vr
from .conftest import load_golden

SCORE_RTOL, SCORE_FLOOR = 1e-4, 1e-2   # the project's score bar (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def relerr(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), SCORE_FLOOR)))


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------

def test_view_rotations_argument_validation_needs_no_gpu(lib):
    err = lib.ahv_last_error
    vrot = lib.ahv_view_rotations_f32   # (Q, q_batch_stride, A, B, V, N, out, stream)
    for bad in (0, 17, -1):
        assert vrot(1, 0, 1, 1, bad, 10, 1, None) == -1 and b"V = " in err() and str(bad).encode() in err()
    assert vrot(1, 0, 1, 0, 3, 10, 1, None) == -1 and b"at least 1" in err()
    assert vrot(1, 0, 1, 1, 3, 0, 1, None) == -1 and b"at least 1" in err()
    assert vrot(1, 0, 1, -1, 3, 10, 1, None) == -1 and b"at least 1" in err()
    assert vrot(1, 0, 1, 65536, 3, 10, 1, None) == -1 and b"65535" in err()
    for bad in (5, 89, 91, -90):
        assert vrot(1, bad, 1, 1, 3, 10, 1, None) == -1 and b"q_batch_stride" in err()
    assert vrot(None, 0, 1, 1, 3, 10, 1, None) == -1 and b"null" in err()
    assert vrot(1, 0, None, 1, 3, 10, 1, None) == -1 and b"null" in err()
    assert vrot(1, 0, 1, 1, 3, 10, None, None) == -1 and b"null" in err()
    assert vrot(1, 0, 1, 1, 3, (1 << 32) + 1, 1, None) == -1 and b"32 bits" in err()
    assert vrot(1, 0, 1, 65535, 16, 1 << 30, 1, None) == -1 and b"one launch" in err()


def test_fuse_view_scores_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    L = ahv._lib
    fuse = lib.ahv_fuse_view_scores_f32
    tau = float(vr.tau_of(60.0))
    # (scores, Q, q_batch_stride, A, weights, B, V, N, n_offset, min_trace, fused, best_key, flags, stream)
    ok = [1, 1, 0, 1, None, 1, 3, 10, 0, tau, 1, 1, 0, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fuse(*a)

    for bad in (0, 17, -1):
        assert call(_6=bad) == -1 and b"V = " in err() and str(bad).encode() in err()
    assert call(_5=0) == -1 and b"at least 1" in err()
    assert call(_7=0) == -1 and b"at least 1" in err()
    assert call(_7=-3) == -1 and b"at least 1" in err()
    assert call(_5=65536) == -1 and b"65535" in err()
    assert call(_8=1 << 32) == -1 and b"32 bits" in err()
    assert call(_8=-1) == -1 and b"32 bits" in err()
    for bad in (8, 4, 128):
        assert call(_12=bad) == -1 and b"flags" in err()
    for bad in (-1.0, 3.0, float("nan"), float("inf"), -float("inf"), 3.5, -1.5):
        assert call(_9=bad) == -1 and b"min_trace" in err(), bad
    for bad in (5, 89, 91, -90):
        assert call(_2=bad) == -1 and b"q_batch_stride" in err()
    assert call(_0=None) == -1 and b"null" in err()
    assert call(_11=None) == -1 and b"null" in err()
    assert call(_1=None) == -1 and b"null" in err()     # an angle limit needs Q ...
    assert call(_3=None) == -1 and b"null" in err()     # ... and A
    W = lambda *v: (ctypes.c_float * len(v))(*v)
    for bad in (W(1.0, -0.5, 1.0), W(1.0, float("nan"), 1.0), W(float("inf"), 1.0, 1.0)):
        assert call(_4=bad) == -1 and b"weights[" in err() and b"finite" in err()
    assert call(_4=W(0.0, 0.0, 0.0)) == -1 and b"all zero" in err()
    assert call(_4=W(0.0, -0.0, 0.0)) == -1 and b"all zero" in err()
    assert (L.AHV_VIEWS_MAX, L.AHV_VIEWS_RESET_BEST, L.AHV_VIEWS_NO_ANGLE_LIMIT) == (16, 1, 2)
    assert lib.ahv_abi_version() == (2 << 16) | 3   # added under 2.3: callers probe for the symbol


def test_views_ops_refuse_cpu_tensors_and_bad_shapes(ahv):
    ops = ahv.ops
    Q = torch.eye(3)[None].repeat(8, 1, 1)
    A = torch.eye(3)[None, None].repeat(2, 3, 1, 1)
    s = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_rotations(Q, A)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fuse_view_scores(s, Q, A)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.verify_views(torch.zeros(2, 3, 16, 8, 8, 8), torch.zeros(2, 16, 8, 8, 8), Q, A, torch.zeros(32, 384),
                         torch.zeros(32, 32), torch.zeros(32))
    with pytest.raises(RuntimeError, match="V = 17"):
        ops.fuse_view_scores(torch.zeros(2, 17, 8), Q, torch.eye(3)[None, None].repeat(2, 17, 1, 1))
    with pytest.raises(RuntimeError, match=r"\(B,V,N\)"):
        ops.fuse_view_scores(torch.zeros(2, 3, 9), Q, A)
    with pytest.raises(RuntimeError, match="Q must be"):
        ops.view_rotations(torch.eye(3)[None, None].repeat(3, 8, 1, 1), A)
    with pytest.raises(RuntimeError, match="A must be"):
        ops.view_rotations(Q, A[0])
    for bad in (0.0, 180.0, float("nan")):
        with pytest.raises(RuntimeError, match="min_angle_deg"):
            ops.fuse_view_scores(s, Q, A, max_view_angle_deg=bad)
    with pytest.raises(RuntimeError, match="weights must hold"):
        ops.fuse_view_scores(s, Q, A, weights=[1.0, 1.0])
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.fuse_view_scores(s.requires_grad_(True), Q, A)
    with pytest.raises(RuntimeError, match="vol_refs"):
        ops.verify_views(torch.zeros(2, 2, 16, 8, 8, 8), torch.zeros(2, 16, 8, 8, 8), Q, A, torch.zeros(32, 384),
                         torch.zeros(32, 32), torch.zeros(32))
    assert ops.min_trace(60.0) == float(vr.tau_of(60.0))


def test_aligner_verify_views_follows_the_inference_rule(ahv):
    fa = ahv.aligner.Feature_Aligner(in_channel=64, mid_channel=32, out_channel=32, n_heads=4, depth=1)
    Q = torch.eye(3)[None].repeat(8, 1, 1)
    A = torch.eye(3)[None, None].repeat(1, 2, 1, 1)
    refs, query = torch.zeros(1, 2, 16, 8, 8, 8), torch.zeros(1, 16, 8, 8, 8)
    fa.train()
    with pytest.raises(RuntimeError, match="inference step"):
        fa.verify_views(refs, query, Q, A)
    fa.eval()   # grad mode on, parameters require grad: still an inference call -- and the op layer then wants the GPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.verify_views(refs, query, Q, A)


# ---- the reference against the fixture of the reference's own code --------------------------------------------

def test_reference_against_the_multiview_fixture():
    from oracle import torch_ref
    g = load_golden("multiview")
    B, V, N = g["scores"].shape
    assert (B, V, N) == (2, 3, 40) and float(g["margin"].min()) >= 1e-3
    R = vr.view_rotations(g["Q"], g["A"])
    assert np.max(np.abs(R - g["R"])) <= 1e-6                                  # Q_n A_v^T as the generator formed it in torch
    W1, W2, b2 = (torch.from_numpy(g[k]) for k in ("W1", "W2", "b2"))
    for b in range(B):
        for v in range(V):      # per-view scores through the stock-torch restatement of the reference's op sequence
            s, _, _ = torch_ref.score_hypotheses(torch.from_numpy(g["vol_refs"][b, v][None]), torch.from_numpy(g["vol_query"][b][None]),
                                                 torch.from_numpy(g["R"][b, v]), W1, W2, b2)
            assert relerr(s.numpy()[0], g["scores"][b, v]) <= SCORE_RTOL, (b, v)
    S, scale, part, margin = vr.fuse(g["scores"], g["Q"], g["A"])
    assert part.all() and margin == np.inf
    assert np.max(np.abs(S - g["fused"])) <= 1e-5
    score, idx = vr.decode(vr.best_keys(S))
    assert idx.tolist() == g["best_idx"].tolist() == g["plant"].tolist()        # exact: the lead is >= 1e-3
    assert np.max(np.abs(score - g["best"])) <= 1e-5
    # every view alone already prefers the planted pose; so does any weighting of them
    for w in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [0.2, 0.5, 3.0]):
        assert vr.decode(vr.best_keys(vr.fuse(g["scores"], g["Q"], g["A"], w)[0]))[1].tolist() == g["plant"].tolist()


# ---- hand cases of the reference ------------------------------------------------------------------------------

def _haar(ahv, n, seed):
    return ahv.rotations.haar_rotations_np(n, seed=seed)


def test_one_view_is_the_single_pair_argmax(ahv):
    rng = np.random.default_rng(5)
    s = rng.standard_normal((3, 1, 200)).astype(np.float32)
    s[0, 0, 17] = s[0, 0, 90] = s[0].max() + 1          # a tie: the lowest index
    s[1, 0, 5], s[2, 0, 7], s[2, 0, 9] = np.nan, np.inf, -np.inf
    Q, A = _haar(ahv, 200, 1), _haar(ahv, 3, 2).reshape(3, 1, 3, 3)
    for w in (None, [0.37]):
        S, scale, g, _ = vr.fuse(s, Q, A, w)
        fin = np.isfinite(s[:, 0])
        assert w is not None or np.array_equal(S[fin], s[:, 0][fin].astype(np.float64))   # one view, weight 1: the score itself
        assert np.allclose(S[fin], s[:, 0][fin], rtol=1e-15) and np.array_equal(np.isnan(S), np.isnan(s[:, 0]))
        keys = vr.best_keys(S, n_offset=11)
        idx = np.broadcast_to(np.arange(200) + 11, (3, 200))
        assert np.array_equal(keys, ahv.dist.pack_keys_host(s[:, 0], idx).reshape(3, 200).max(axis=1))
        assert vr.decode(keys)[1].tolist() == [17 + 11, 5 + 11, 7 + 11]         # tie -> lowest index; NaN above +inf


def test_a_zero_weight_view_with_nan_scores_is_absent(ahv):
    rng = np.random.default_rng(6)
    s = rng.standard_normal((2, 3, 50)).astype(np.float32)
    s[:, 1] = np.nan
    Q, A = _haar(ahv, 50, 3), _haar(ahv, 6, 4).reshape(2, 3, 3, 3)
    S, scale, g, _ = vr.fuse(s, Q, A, [1.0, 0.0, 3.0])
    assert np.all(np.isfinite(S)) and not g[:, 1].any() and g[:, 0].all() and g[:, 2].all()
    assert np.allclose(S, (s[:, 0].astype(np.float64) + 3.0 * s[:, 2].astype(np.float64)) / 4.0, rtol=1e-14)
    assert np.all(np.isnan(vr.fuse(s, Q, A, [1.0, 1e-3, 3.0])[0]))              # the same view with any weight: NaN, as torch.sum


def test_a_limit_that_excludes_every_view_gives_minus_inf(ahv):
    Q = _haar(ahv, 64, 7)
    A = np.broadcast_to(np.eye(3, dtype=np.float32), (1, 2, 3, 3))
    ang = np.degrees(np.arccos(np.clip((np.trace(Q, axis1=1, axis2=2) - 1) / 2, -1, 1)))   # relative angle to both views
    theta = float(ang.min()) * 0.5
    s = np.random.default_rng(8).standard_normal((1, 2, 64)).astype(np.float32)
    S, scale, g, margin = vr.fuse(s, Q, A, None, theta)
    assert not g.any() and np.all(S == -np.inf) and np.all(np.isnan(scale)) and margin > 0
    keys = vr.best_keys(S)
    assert keys[0] != vr.EMPTY and vr.decode(keys)[1].tolist() == [0] and vr.decode(keys)[0][0] == -np.inf
    # per hypothesis: only the views within the limit take part
    theta = float(np.median(ang))
    S, scale, g, _ = vr.fuse(s, Q, A, [1.0, 2.0], theta)
    inside = ang <= theta
    assert np.array_equal(g[0, 0], inside) and np.array_equal(g[0, 1], inside)
    assert np.all(S[0, ~inside] == -np.inf) and np.allclose(S[0, inside], ((s[0, 0].astype(np.float64) + 2.0 * s[0, 1].astype(np.float64)) / 3.0)[inside])


def test_a_nan_entry_in_a_hypothesis_takes_it_out_under_a_limit(ahv):
    Q = _haar(ahv, 16, 9)
    Q[:] = Q[0]                                       # every hypothesis sits on view 0's pose
    A = Q[:1].reshape(1, 1, 3, 3).copy()
    Q[5, 1, 2] = np.nan
    s = np.ones((1, 1, 16), np.float32)
    S, _, g, _ = vr.fuse(s, Q, A, None, 60.0)
    assert S[0, 5] == -np.inf and not g[0, 0, 5] and np.all(np.delete(S[0], 5) == 1.0)
    assert np.all(vr.fuse(s, Q, A)[0] == 1.0)         # without a limit Q is not looked at
