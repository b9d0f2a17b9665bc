"""Gradient-based pose polishing: the SO(3) ascent kernels against their host mirror (rotations.so3_ascent_*),
ops.polish_rotations, ops.verify_pair_polished and CoarseToFine(polish_iters=...).

Planted optimum (test_planted_optimum): vol_tgt := rotate_volume(vol_src, R_gt) makes score(R_gt) = 1 the global maximum for
any weights.  Seeds R_gt exp([d]x), |d| in PLANTED_DEG, four axes per size, two R_gt.  The yardstick is the fp64 CPU mirror of
the same algorithm (torch autograd gradient + rotations.so3_ascent_*), run inside the test.  Sizes kept: those from which the
mirror ends closer to R_gt than it started for EVERY seed (``python -m tests.test_gpu_polish`` prints the mirror's table, no
GPU needed) -- see PLANTED_DEG below for the sizes and the mirror's errors before and after."""
import math

import numpy as np
import pytest
import torch

from .conftest import load_golden
from .test_gpu_rotation_grad import ref_rotation_grad

pytestmark = pytest.mark.gpu
SCORE_RTOL, SCORE_FLOOR = 1e-4, 1e-2
LADDER = (0.25, 0.5, 1.0, 2.0)
# The mirror (fp64, 8 iterations, default ladder and angle), geodesic error to R_gt in degrees, worst seed of each size:
#   0.5 -> 1.4e-2   1 -> 9.4e-3   2 -> 5.2e-3   3 -> 1.1e-2   (every seed of every size ends closer than it started; final
#   score 1.00000000 from every seed).  The fp32 kernels on the MI355X end within 2.4e-2 from every seed, score 1.000000.
PLANTED_DEG = (0.5, 1.0, 2.0, 3.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def head():
    g = load_golden("score_n128")
    return _t(g["W1"]), _t(g["W2"]), _t(g["b2"])


# ---- 5. step kernels against the host mirror ---------------------------------------------------------
def test_candidates_match_the_mirror(ahv, ops, dev):
    rot = ahv.rotations
    B, K = 3, 7
    R = _t(rot.haar_rotations_np(B * K, 5)).reshape(B, K, 3, 3)
    G = torch.randn(B, K, 3, 3, generator=torch.Generator().manual_seed(1))
    G[0, 2] = 0                                   # zero direction
    G[2, 1, 0, 0] = float("nan")                  # non-finite direction
    theta = torch.rand(B, K, generator=torch.Generator().manual_seed(2)) * 0.1 + 1e-3
    for ladder in (LADDER, (0.5,), (0.1, 0.3, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0)):
        want = rot.so3_ascent_candidates(R.double(), G.double(), theta.double(), ladder)
        got = ops.so3_ascent_candidates(R.to(dev), G.to(dev), theta.to(dev), ladder).cpu()
        L = len(ladder)
        assert tuple(got.shape) == (B, K * (L + 1), 3, 3)
        assert (got.double() - want).abs().max().item() <= 1e-6
        slots = got.reshape(B, K, L + 1, 3, 3)
        assert torch.equal(slots[:, :, 0], R)
        for b, k in ((0, 2), (2, 1)):
            assert torch.equal(slots[b, k], R[b, k].expand(L + 1, 3, 3))


def test_selection_matches_the_mirror(ahv, ops, dev):
    rot = ahv.rotations
    B, K, L = 2, 6, len(LADDER)
    gen = torch.Generator().manual_seed(3)
    cand = torch.randn(B, K * (L + 1), 3, 3, generator=gen)
    sc = torch.randn(B, K, L + 1, generator=gen)
    nan = float("nan")
    sc[0, 0] = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5])        # all equal: slot 0 stays
    sc[0, 1] = torch.tensor([0.1, 0.7, 0.7, 0.2, 0.7])        # tie between candidates: the earliest
    sc[0, 2] = torch.tensor([0.3, nan, 0.2, nan, 0.25])       # NaN never replaces
    sc[0, 3] = torch.tensor([nan, 0.9, 0.8, 0.7, 0.6])        # a NaN incumbent stays (nothing compares greater)
    sc[0, 4] = torch.tensor([0.3, 0.2, 0.4, nan, 0.5])
    sc[1, 0] = torch.tensor([0.3, 0.3, 0.2, 0.1, 0.0])        # tie with the incumbent: slot 0 wins
    sc = sc.reshape(B, K * (L + 1))
    theta = torch.rand(B, K, generator=gen) * 0.05 + 0.01
    want_R, want_s, want_t = rot.so3_ascent_select(cand, sc, theta, LADDER)
    R_cur = torch.zeros(B, K, 3, 3, device=dev)
    s_cur = torch.zeros(B, K, device=dev)
    th = theta.to(dev)
    ops.so3_ascent_select(cand.to(dev), sc.to(dev), LADDER, R_cur, s_cur, th)
    assert torch.equal(R_cur.cpu(), want_R)
    assert torch.equal(s_cur.cpu().nan_to_num(nan=-7.0), want_s.nan_to_num(nan=-7.0))
    assert torch.equal(th.cpu(), want_t)                      # exact: one fp32 product either way
    slots = [0, 1, 0, 0, 4, 0]
    lad = torch.tensor((min(LADDER),) + LADDER)
    assert torch.equal(want_t[0], theta[0] * lad[slots]) and torch.equal(want_t[1, 0], theta[1, 0] * min(LADDER))


# ---- 6. monotone, honest, orthonormal ------------------------------------------------------------------
def _fixture_seeds(ops, dev, which, K=16):
    W1, W2, b2 = (x.to(dev) for x in head())
    if which == "score_n128":
        g = load_golden("score_n128")
        vs, vt, R = _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev), _t(g["R"]).to(dev)
    else:
        g = load_golden("batched")
        vs, vt = _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev)
        R = _t(g["R_per"] if which == "batched_per" else g["R_shared"]).to(dev)
    scores, _, keys, ft = ops.verify_pair_topk(vs, vt, R, W1, W2, b2, K, want_feat_tgt=True)
    seed_scores, _, R0 = ops.select_topk(keys, R)
    return vs, ft, R0, seed_scores, (W1, W2, b2)


@pytest.mark.parametrize("which", ["score_n128", "batched_shared", "batched_per"])
def test_polish_is_monotone_honest_orthonormal(ops, dev, which):
    vs, ft, R0, seed_scores, w = _fixture_seeds(ops, dev, which)
    R, s, theta = ops.polish_rotations(vs, ft, R0, *w, iters=8)
    print(which, "seed scores", seed_scores[0, :4].tolist(), "-> polished", s[0, :4].tolist(),
          "moved deg", [round(x, 3) for x in _geo(R, R0)[0, :4].tolist()])
    assert (s >= seed_scores).all()
    assert (s > seed_scores).any()                       # the gradient is worth something on these fixtures
    assert torch.equal(s, ops.score_hypotheses(vs, ft, R, *w)[0])
    eye = torch.eye(3, device=dev)
    assert ((R.transpose(-1, -2) @ R) - eye).abs().max().item() <= 1e-5
    assert (theta > 0).all()
    Rz, sz, _ = ops.polish_rotations(vs, ft, R0, *w, iters=0)
    assert torch.equal(Rz, R0) and torch.equal(sz, seed_scores)
    R2, s2, t2 = ops.polish_rotations(vs, ft, R0, *w, iters=8)
    assert torch.equal(R2, R) and torch.equal(s2, s) and torch.equal(t2, theta)
    # graph replay: static buffers, no allocation inside the captured call
    buf = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.polish_rotations(vs, ft, R0, *w, iters=8, out=buf)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.polish_rotations(vs, ft, R0, *w, iters=8, out=buf)
    for o in out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], R) and torch.equal(out[1], s) and torch.equal(out[2], theta)


def _geo(a, b):
    from importlib import import_module
    return import_module("3dahv_amd").rotations.geodesic_deg(a.double().cpu(), b.double().cpu()).reshape(a.shape[:-2])


# ---- 7. planted optimum ------------------------------------------------------------------------------
def planted_case(ahv):
    """(vol_src (2,...), vol_tgt (2,...), R_gt64 (2,3,3) orthonormal in fp64, seeds (2,K,3,3) fp32, sizes (K,))."""
    from oracle import torch_ref
    rot = ahv.rotations
    g = load_golden("score_n128")
    vs = _t(g["vol_src"]).expand(2, -1, -1, -1, -1).contiguous()
    U, _, Vh = torch.linalg.svd(_t(rot.haar_rotations_np(2, 4242)).double())
    R_gt = U @ Vh
    with torch.no_grad():
        vt = torch.cat([torch_ref.rotate_volume(vs[b:b + 1], R_gt[b:b + 1].float()) for b in range(2)]).contiguous()
    axes = torch.tensor([[1.0, 0.3, -0.2], [-0.4, 1.0, 0.5], [0.2, -0.6, 1.0], [-1.0, -1.0, 0.7]], dtype=torch.float64)
    axes = axes / axes.norm(dim=1, keepdim=True)
    sizes = torch.tensor([d for d in PLANTED_DEG for _ in range(len(axes))], dtype=torch.float64)
    w = axes.repeat(len(PLANTED_DEG), 1) * torch.deg2rad(sizes)[:, None]
    seeds = (R_gt[:, None] @ rot.axis_angle_to_matrix(w)[None]).float()
    return vs, vt, R_gt, seeds, sizes


def mirror_polish(ahv, vs, vt, R0, W1, W2, b2, iters=8, init_angle_deg=2.0, ladder=LADDER):
    """ops.polish_rotations restated in fp64 on the CPU: torch autograd gradient + rotations.so3_ascent_*."""
    from oracle import torch_ref
    from .test_gpu_backward import ref_scores
    rot = ahv.rotations
    d = lambda x: x.detach().cpu().double()
    vs, vt, R, W1, W2, b2 = d(vs), d(vt), d(R0), d(W1), d(W2), d(b2)
    with torch.no_grad():
        ft = torch_ref.forward_3d2d(vt, W1, W2, b2)
    B, K = R.shape[:2]
    theta = torch.full((B, K), math.radians(init_angle_deg), dtype=torch.float64)
    with torch.no_grad():
        s = ref_scores(vs, ft, R, W1, W2, b2)
    for _ in range(iters):
        G, _ = ref_rotation_grad(vs, ft, R, W1, W2, b2)
        cand = rot.so3_ascent_candidates(R, G, theta, ladder)
        with torch.no_grad():
            cs = ref_scores(vs, ft, cand, W1, W2, b2)
        R, s, theta = rot.so3_ascent_select(cand, cs, theta, ladder)
    return R, s


def test_planted_optimum(ahv, ops, dev):
    vs, vt, R_gt, seeds, sizes = planted_case(ahv)
    W1, W2, b2 = head()
    Rm, sm = mirror_polish(ahv, vs, vt, seeds, W1, W2, b2)
    before = _geo(seeds, R_gt[:, None].expand_as(seeds))
    after_m = _geo(Rm, R_gt[:, None].expand_as(seeds))
    assert (after_m < before).all(), "the mirror itself must end closer from every seed of the sizes kept"
    g = lambda x: x.to(dev)
    ft = ops.forward_3d2d(g(vt), g(W1), g(W2), g(b2))
    R, s, _ = ops.polish_rotations(g(vs), ft, g(seeds), g(W1), g(W2), g(b2), iters=8)
    after = _geo(R, R_gt[:, None].expand_as(seeds))
    for d in PLANTED_DEG:
        m = sizes == d
        print("seeds at %.1f deg: error before %.4f, mirror after max %.2e, kernel after max %.2e; score mirror min %.6f kernel min %.6f"
              % (d, before[:, m].max(), after_m[:, m].max(), after[:, m].max(), sm[:, m].min(), s[:, m].min()))
    assert (after <= before).all()
    assert (s.cpu().double() >= sm - SCORE_RTOL * sm.abs().clamp_min(SCORE_FLOOR)).all()


# ---- 8. verify_pair_polished, CoarseToFine(polish_iters) -------------------------------------------------
def test_verify_pair_polished(ahv, ops, dev):
    g = load_golden("batched")
    W1, W2, b2 = (x.to(dev) for x in head())
    vs, vt = _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev)
    R = _t(ahv.rotations.haar_rotations_np(3000, 8)).to(dev)
    plain_scores, key = ops.verify_pair(vs, vt, R, W1, W2, b2)
    plain, plain_idx = ops.unpack_best(key)
    for K in (1, 8):
        score, R_pred, seed_idx, info = ops.verify_pair_polished(vs, vt, R, W1, W2, b2, K=K, iters=4)
        _, _, keys = ops.verify_pair_topk(vs, vt, R, W1, W2, b2, K)
        assert torch.equal(info["keys"], keys)
        ts, ti, _ = ops.select_topk(keys, R)
        assert torch.equal(info["topk_scores"], ts) and torch.equal(info["topk_idx"], ti)
        assert torch.equal(ts[:, 0], plain) and torch.equal(ti[:, 0], plain_idx)      # entry 0 IS the unpolished arg-max
        assert (score >= plain).all()
        assert torch.equal(score, info["polished_scores"].max(dim=1).values)
        rows = torch.arange(3, device=dev)
        assert torch.equal(seed_idx, ti[rows, info["seed_rank"]])
        ft = ops.verify_pair(vs, vt, R[:1], W1, W2, b2, want_feat_tgt=True)[2]   # the step's own (in-launch) target features
        assert torch.equal(score, ops.score_hypotheses(vs, ft, R_pred[:, None].contiguous(), W1, W2, b2)[0][:, 0])
    with pytest.raises(RuntimeError, match="no autograd edge"):
        ops.verify_pair_polished(vs.clone().requires_grad_(True), vt, R, W1, W2, b2)
    with pytest.raises(RuntimeError, match="split_f16"):
        ops.verify_pair_polished(vs, vt, R, W1, W2, b2, split_f16=True)
    with ops.split_f16_scorer():
        with pytest.raises(RuntimeError, match="split_f16"):
            ops.verify_pair_polished(vs, vt, R, W1, W2, b2)


def test_coarse_to_fine_polish(ahv, ops, dev):
    g = load_golden("batched")
    W1, W2, b2 = (x.to(dev) for x in head())
    vs, vt = _t(g["vol_src"]).to(dev), _t(g["vol_tgt"]).to(dev)
    R = _t(ahv.rotations.haar_rotations_np(2000, 9)).to(dev)
    C = ahv.refine.CoarseToFine
    base = [x.clone() for x in C(W1, W2, b2, R, n_fine=200, batch=3, use_graph=False)(vs, vt)]
    zero = C(W1, W2, b2, R, n_fine=200, batch=3, use_graph=False, polish_iters=0)(vs, vt)
    for a, b in zip(base, zero):
        assert torch.equal(a, b)
    for kw in ({"use_graph": False}, {"use_graph": True}, {"use_graph": False, "seeds": 4}):
        c2f = C(W1, W2, b2, R, n_fine=200, batch=3, polish_iters=4, **kw)
        out = [x.clone() for x in c2f(vs, vt)]
        if "seeds" not in kw:
            assert torch.equal(out[1], base[1]) and torch.equal(out[3], base[3]) and torch.equal(out[4], base[4])
            assert (out[0] >= base[0]).all()
            assert torch.equal(c2f.last["polish"]["score_before"], base[0])
            assert torch.equal(c2f.last["polish"]["R_before"], base[2])
        assert (out[0] >= c2f.last["polish"]["score_before"]).all()
        ft = ops.verify_pair(vs, vt, R[:1], W1, W2, b2, want_feat_tgt=True)[2]   # the step's own (in-launch) target features
        assert torch.equal(out[0], ops.score_hypotheses(vs, ft, out[2][:, None].contiguous(), W1, W2, b2)[0][:, 0])
        if kw.get("use_graph"):
            again = [x.clone() for x in c2f(vs, vt)]
            for a, b in zip(out, again):
                assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="fused"):
        C(W1, W2, b2, R, n_fine=200, batch=3, fused=True, polish_iters=2)


def test_run_many_with_polishing_replays_from_one_graph(ahv, ops, dev):
    """Three steps captured into one graph: slots 1 and 2 get their polishing buffers like slot 0, and every captured step
    equals the eager step on the same pair."""
    g = load_golden("batched")
    W1, W2, b2 = (x.to(dev) for x in head())
    R = _t(ahv.rotations.haar_rotations_np(2000, 9)).to(dev)
    vs = _t(g["vol_src"]).to(dev)[:, None].contiguous()      # (steps = 3, B = 1, ...)
    vt = _t(g["vol_tgt"]).to(dev)[:, None].contiguous()
    C = ahv.refine.CoarseToFine
    eager = C(W1, W2, b2, R, n_fine=200, batch=1, use_graph=False, polish_iters=3)
    want = [[x.clone() for x in eager(vs[k], vt[k])] for k in range(3)]
    many = C(W1, W2, b2, R, n_fine=200, batch=1, use_graph=True, polish_iters=3)
    for _ in range(2):   # capture, then a second replay
        got = many.run_many(vs, vt, steps=3)
        torch.cuda.synchronize()
        for k in range(3):
            for a, b in zip(got[k], want[k]):
                assert torch.equal(a, b), k
    # a ladder handed over as a device tensor is used as it is
    lad = torch.tensor(LADDER, device=dev)
    f = ops.verify_pair(vs[0], vt[0], R[:1], W1, W2, b2, want_feat_tgt=True)[2]
    a = ops.polish_rotations(vs[0], f, want[0][2][:, None].contiguous(), W1, W2, b2, iters=2, ladder=lad)
    b = ops.polish_rotations(vs[0], f, want[0][2][:, None].contiguous(), W1, W2, b2, iters=2, ladder=LADDER)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


_RCCL_SCRIPT = r'''
import importlib, os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
ahv = importlib.import_module("3dahv_amd")
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", sys.argv[2])
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "batched.npz")); h = np.load(os.path.join(sys.argv[1], "tests", "golden", "score_n128.npz"))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
vs, vt, W1, W2, b2 = T(g["vol_src"]), T(g["vol_tgt"]), T(h["W1"]), T(h["W2"]), T(h["b2"])
R = T(ahv.rotations.haar_rotations_np(2000, 9))
plain = [x.clone() for x in ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=200, batch=3, use_graph=False, polish_iters=4)(vs, vt)]
calls = []
real = dist.all_reduce
dist.all_reduce = lambda t, *a, **k: (calls.append(tuple(t.shape)), real(t, *a, **k))[1]
eager = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=200, batch=3, use_graph=False, polish_iters=4, force_collectives=True)
out = [x.clone() for x in eager(vs, vt)]
assert calls == [(3,), (3,)], calls          # still two collectives per step
for a, b in zip(out, plain):
    assert torch.equal(a, b)
graphed = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=200, batch=3, polish_iters=4, force_collectives=True)
assert graphed.use_graph
out = [x.clone() for x in graphed(vs, vt)]
torch.cuda.synchronize()
for a, b in zip(out, plain):
    assert torch.equal(a, b)
dist.destroy_process_group()
print("POLISH_RCCL_OK")
'''


def test_polish_keeps_two_collectives_under_rccl(tmp_path):
    """A forced one-rank RCCL group, in a fresh child process (the process group must not leak into this one)."""
    import subprocess
    import sys
    from .conftest import REPO
    from .test_dist_cpu import _free_port
    script = tmp_path / "polish_rccl.py"
    script.write_text(_RCCL_SCRIPT)
    p = subprocess.run([sys.executable, str(script), REPO, str(_free_port())], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0 and "POLISH_RCCL_OK" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":   # the mirror's table for PLANTED_DEG (no GPU)
    import importlib
    pkg = importlib.import_module("3dahv_amd")
    vs, vt, R_gt, seeds, sizes = planted_case(pkg)
    Rm, sm = mirror_polish(pkg, vs, vt, seeds, *head())
    before, after = _geo(seeds, R_gt[:, None].expand_as(seeds)), _geo(Rm, R_gt[:, None].expand_as(seeds))
    for d in sorted(set(sizes.tolist())):
        m = sizes == d
        print("%.1f deg: before %s after max %.2e, all closer: %s, final score min %.8f"
              % (d, [round(x, 3) for x in before[:, m].flatten().tolist()[:2]], after[:, m].max(), bool((after[:, m] < before[:, m]).all()),
                 sm[:, m].min()))
