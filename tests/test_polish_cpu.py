"""Pose polishing without a GPU: properties of the host mirror of the SO(3) ascent step (rotations.so3_ascent_*), the
argument validation of the three new entry points (before any HIP call, as in test_abi.py), and the multi-rank control flow
of ``CoarseToFine(polish_iters=2)`` under world-2 gloo on an oracle-backed CPU backend whose rotation gradient is torch
autograd and whose ascent steps are the host mirror: both ranks return the same ``R_pred`` as a single rank, with the two
collectives of the unpolished step."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .conftest import REPO
from .test_dist_cpu import _free_port
from .test_refine_dist_cpu import OracleBackend, _inputs, N_COARSE, N_FINE

LADDER = (0.25, 0.5, 1.0, 2.0)


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


# ---- the host mirror -----------------------------------------------------------------------------------
def _seeds(ahv, B=2, K=5, seed=0):
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(B * K, seed)).double().reshape(B, K, 3, 3)
    G = torch.randn(B, K, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    theta = torch.full((B, K), math.radians(2.0), dtype=torch.float64)
    return R, G, theta


def test_tangent_is_skew_and_is_the_directional_derivative(ahv):
    rot = ahv.rotations
    R, G, _ = _seeds(ahv)
    S = rot.so3_tangent(R, G)
    assert torch.equal(S, -S.transpose(-1, -2))
    # f(R) = <G, R>: d/de f(R exp(e [w]x)) at 0 equals 2 <vee(S), w>
    w = torch.randn(2, 5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    e = 1e-6
    step = rot.axis_angle_to_matrix((w * e).reshape(-1, 3)).reshape(2, 5, 3, 3)
    num = ((G * (R @ step)).sum((-1, -2)) - (G * R).sum((-1, -2))) / e
    vee = torch.stack([S[..., 2, 1], S[..., 0, 2], S[..., 1, 0]], dim=-1)
    assert torch.allclose(num, 2 * (vee * w).sum(-1), atol=1e-4)


def test_candidates_are_rotations_at_the_ladder_angles(ahv):
    rot = ahv.rotations
    R, G, theta = _seeds(ahv)
    U, _, Vh = torch.linalg.svd(R)
    R = U @ Vh
    cand = rot.so3_ascent_candidates(R, G, theta, LADDER)
    assert tuple(cand.shape) == (2, 5 * 5, 3, 3)
    assert (cand.transpose(-1, -2) @ cand - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12
    assert torch.allclose(torch.linalg.det(cand), torch.ones(2, 25, dtype=torch.float64))
    slots = cand.reshape(2, 5, 5, 3, 3)
    assert torch.equal(slots[:, :, 0], R)
    ang = rot.geodesic_deg(slots[:, :, 1:], R[:, :, None].expand(2, 5, 4, 3, 3)).reshape(2, 5, 4)
    assert torch.allclose(ang, 2.0 * torch.tensor(LADDER, dtype=torch.float64).expand(2, 5, 4), atol=1e-5)
    # first-order ascent of f(R) = <G, R> along every candidate
    f = lambda X: (G[:, :, None] * X).sum((-1, -2))
    assert (f(slots[:, :, 1:]) > f(slots[:, :, :1])).all()


def test_zero_or_non_finite_direction_keeps_the_seed(ahv):
    rot = ahv.rotations
    R, G, theta = _seeds(ahv)
    G[0, 0] = 0
    G[0, 1] = R[0, 1] * 3.0                      # R^T G = 3 I: symmetric, no tangent part
    G[1, 2, 1, 1] = float("inf")
    G[1, 3, 0, 2] = float("nan")
    slots = rot.so3_ascent_candidates(R, G, theta, LADDER).reshape(2, 5, 5, 3, 3)
    for b, k in ((0, 0), (0, 1), (1, 2), (1, 3)):
        assert torch.equal(slots[b, k], R[b, k].expand(5, 3, 3))
    assert not torch.equal(slots[1, 4, 1], R[1, 4])


def test_selection_rules(ahv):
    rot = ahv.rotations
    nan = float("nan")
    sc = torch.tensor([[[0.5, 0.5, 0.5, 0.5, 0.5],       # all equal: slot 0
                        [0.1, 0.7, 0.7, 0.2, 0.7],       # tie between candidates: the earliest
                        [0.3, nan, 0.2, nan, 0.25],      # NaN never replaces
                        [nan, 0.9, 0.8, 0.7, 0.6],       # a NaN incumbent stays
                        [0.3, 0.2, 0.4, nan, 0.5]]], dtype=torch.float64)
    cand = torch.arange(25 * 9, dtype=torch.float64).reshape(1, 25, 3, 3)
    theta = torch.tensor([[0.04, 0.03, 0.02, 0.01, 0.05]], dtype=torch.float64)
    R, s, t = rot.so3_ascent_select(cand, sc.reshape(1, 25), theta, LADDER)
    slots = [0, 1, 0, 0, 4]
    assert torch.equal(R[0], torch.stack([cand[0, 5 * k + l] for k, l in enumerate(slots)]))
    assert torch.equal(s[0].nan_to_num(nan=-1.0), torch.tensor([0.5, 0.7, 0.3, -1.0, 0.5], dtype=torch.float64))
    assert torch.equal(t[0], theta[0] * torch.tensor([0.25, 0.25, 0.25, 0.25, 2.0], dtype=torch.float64))
    # the score of a seed never decreases, whatever the candidates' scores
    rnd = torch.randn(4, 6, 5, generator=torch.Generator().manual_seed(4))
    _, best, _ = rot.so3_ascent_select(torch.zeros(4, 30, 3, 3), rnd.reshape(4, 30), torch.ones(4, 6), LADDER)
    assert (best >= rnd[..., 0]).all() and torch.equal(best, rnd.max(dim=-1).values)


# ---- ABI validation (no GPU: it happens before any HIP call) ------------------------------------------------
def test_rotation_grad_validation(lib):
    f = lib.ahv_score_rotation_grad_f32
    assert lib.ahv_score_rotation_grad_workspace_bytes(2, 10) == 2 * 10 * 8192
    assert lib.ahv_score_rotation_grad_workspace_bytes(0, 10) == 0 and lib.ahv_score_rotation_grad_workspace_bytes(3, 0) == 0
    need = 3 * 8192
    assert f(None, None, None, 0, None, None, None, 0, 5, None, None, 0, None, None) == 0      # B == 0
    assert f(None, None, None, 0, None, None, None, 2, 0, None, None, 0, None, None) == 0      # N == 0
    assert f(16, 16, 16, 0, 16, 16, 16, -1, 3, None, 16, need, 16, None) == -1 and b"negative" in lib.ahv_last_error()
    assert f(16, 16, 16, 0, 16, 16, 16, 1, 3, None, 16, need, None, None) == -1 and b"null" in lib.ahv_last_error()
    assert f(None, 16, 16, 0, 16, 16, 16, 1, 3, None, 16, need, 16, None) == -1 and b"null" in lib.ahv_last_error()
    assert f(16, 16, 16, 0, 16, 16, 16, 1, 3, None, None, need, 16, None) == -1 and b"null" in lib.ahv_last_error()
    assert f(16, 16, 16, 5, 16, 16, 16, 1, 3, None, 16, need, 16, None) == -1 and b"r_batch_stride" in lib.ahv_last_error()
    assert f(16, 16, 16, 28, 16, 16, 16, 1, 3, None, 16, need, 16, None) == -1 and b"r_batch_stride" in lib.ahv_last_error()
    assert f(16, 16, 16, 27, 16, 16, 16, 1, 3, None, 16, need - 1, 16, None) == -1 and b"workspace" in lib.ahv_last_error()
    assert f(16, 16, 16, 0, 16, 16, 16, 1, 3, None, 24, need, 16, None) == -1 and b"16-byte aligned" in lib.ahv_last_error()


def test_so3_ascent_validation(lib, ahv):
    c, s = lib.ahv_so3_ascent_candidates_f32, lib.ahv_so3_ascent_select_f32
    max_l, max_k = ahv._lib.AHV_SO3_MAX_LADDER, ahv._lib.AHV_TOPK_MAX_K
    for L in (0, -1, max_l + 1):
        assert c(16, 16, 16, 16, L, 1, 1, 16, None) == -1 and b"L =" in lib.ahv_last_error()
        assert s(16, 16, 16, L, 1, 1, 16, 16, 16, None) == -1 and b"L =" in lib.ahv_last_error()
    for K in (0, -3, max_k + 1):
        assert c(16, 16, 16, 16, 4, 1, K, 16, None) == -1 and b"K =" in lib.ahv_last_error()
        assert s(16, 16, 16, 4, 1, K, 16, 16, 16, None) == -1 and b"K =" in lib.ahv_last_error()
    assert c(16, 16, 16, 16, 4, -1, 1, 16, None) == -1 and b"negative" in lib.ahv_last_error()
    assert c(16, 16, 16, 16, 4, 65536, 1, 16, None) == -1 and b"65535" in lib.ahv_last_error()
    assert s(16, 16, 16, 4, 65536, 1, 16, 16, 16, None) == -1 and b"65535" in lib.ahv_last_error()
    assert c(16, 16, 16, 16, 4, 0, 1, 16, None) == 0 and s(16, 16, 16, 4, 0, 1, 16, 16, 16, None) == 0
    assert c(16, None, 16, 16, 4, 1, 1, 16, None) == -1 and b"null" in lib.ahv_last_error()
    assert c(16, 16, 16, 16, 4, 1, 1, None, None) == -1 and b"null" in lib.ahv_last_error()
    assert s(16, None, 16, 4, 1, 1, 16, 16, 16, None) == -1 and b"null" in lib.ahv_last_error()
    assert s(16, 16, 16, 4, 1, 1, 16, 16, None, None) == -1 and b"null" in lib.ahv_last_error()


def test_ops_refuse_cpu_tensors_and_gradients(ahv):
    ops = ahv.ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.score_rotation_grad(z(1, 16, 8, 8, 8), z(1, 32, 64), z(2, 3, 3), z(32, 384), z(32, 32), z(32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.polish_rotations(z(1, 16, 8, 8, 8), z(1, 32, 64), z(1, 2, 3, 3), z(32, 384), z(32, 32), z(32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.so3_ascent_candidates(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2), LADDER)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.verify_pair(z(1, 16, 8, 8, 8), z(1, 16, 8, 8, 8), z(2, 3, 3).requires_grad_(True), z(32, 384), z(32, 32), z(32))
    with pytest.raises(RuntimeError, match="fused"):
        ahv.refine.CoarseToFine(z(32, 384), z(32, 32), z(32), z(8, 3, 3), n_fine=4, fused=True, polish_iters=1)


# ---- CoarseToFine(polish_iters=2) on two gloo ranks ------------------------------------------------------
class PolishingOracleBackend(OracleBackend):
    """OracleBackend + the polishing ops: the rotation gradient by torch autograd through oracle/torch_ref.py (the oracle's
    "features" are the target VOLUME, see OracleBackend.verify_pair), the ascent steps by the host mirror."""

    def score_rotation_grad(self, vol_src, vol_tgt, R, W1, W2, b2, grad_scores=None):
        from oracle import torch_ref
        from .test_gpu_backward import ref_scores
        with torch.enable_grad():
            Rl = R.detach().double().requires_grad_(True)
            ft = torch_ref.forward_3d2d(vol_tgt.double(), W1.double(), W2.double(), b2.double())
            s = ref_scores(vol_src.double(), ft, Rl, W1.double(), W2.double(), b2.double())
            (g,) = torch.autograd.grad(s.sum() if grad_scores is None else (s * grad_scores).sum(), Rl)
        return g.float()

    def polish_rotations(self, vol_src, vol_tgt, R0, W1, W2, b2, iters=8, init_angle_deg=2.0, ladder=LADDER, out=None):
        rot = self.ahv.rotations
        B, K = R0.shape[:2]
        R, theta = R0.clone(), torch.full((B, K), math.radians(init_angle_deg), dtype=torch.float32)
        score = lambda X: torch.stack([self.score_hypotheses(vol_src[b:b + 1], vol_tgt[b:b + 1], X[b], W1, W2, b2)[0][0]
                                       for b in range(B)])
        s = score(R)
        for _ in range(iters):
            G = self.score_rotation_grad(vol_src, vol_tgt, R, W1, W2, b2)
            cand = rot.so3_ascent_candidates(R, G, theta, ladder)
            R, s, theta = rot.so3_ascent_select(cand, score(cand), theta, ladder)
        return R, s, theta


def _run(ahv, oracle, polish_iters=2):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3, use_graph=True,
                                  backend=PolishingOracleBackend(ahv, oracle), polish_iters=polish_iters)
    out = [t.clone().numpy() for t in c2f(vs, vt)]
    return c2f, out


def _worker(rank, world, port, q):
    import importlib
    import sys
    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ahv = importlib.import_module("3dahv_amd")
        from oracle import oracle
        calls = []
        real_all_reduce = dist.all_reduce
        dist.all_reduce = lambda t, *a, **k: (calls.append(tuple(t.shape)), real_all_reduce(t, *a, **k))[1]
        try:
            c2f, out = _run(ahv, oracle)
        finally:
            dist.all_reduce = real_all_reduce
        assert c2f.world == world and c2f.collectives
        assert calls == [(3,), (3,)], calls      # polishing adds no exchange
        q.put((rank, out, c2f.last["polish"]["score_before"].numpy()))
    finally:
        dist.destroy_process_group()


def test_coarse_to_fine_polish_world2_equals_single_rank(ahv, oracle):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single, ref = _run(ahv, oracle)
    _, plain = _run(ahv, oracle, polish_iters=0)
    for rank, out, before in got:
        for a, b in zip(out, ref):
            assert np.array_equal(a, b), rank
        assert np.array_equal(before, plain[0])
    assert np.array_equal(ref[1], plain[1]) and np.array_equal(ref[3], plain[3]) and np.array_equal(ref[4], plain[4])
    assert np.all(ref[0] >= plain[0])            # a polished score never falls below the fine winner's
    assert np.any(ref[0] > plain[0])
    Rp = ref[2]
    assert np.allclose(Rp @ Rp.transpose(0, 2, 1), np.eye(3), atol=1e-5)
