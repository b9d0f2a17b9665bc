"""Distinct pose modes on the GPU: ``ahv_topk_modes_f32`` through ``ops.topk_modes`` / ``ops.verify_pair_modes`` against the
numpy reference (tests/modes_reference.py) run on the GPU's own scores, and ``CoarseToFine(modes=K)`` built on it.

Lists are compared as int64 keys with ``torch.equal``.  Every comparison first ASSERTS that the reference's decision margin
(the smallest |t - tau| it met, t in fp64) is at least 1e-4: an fp32 summation-order difference moves t by ~1e-6, so the
kernel's fp32 t cannot flip a decision on such an input.  The seeds below were chosen on the CPU so that it holds (synthetic
scores: the whole reference run needs no GPU); a failing margin means the input is wrong, never the kernel."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import modes_reference as mr
from . import rotation_families
from .conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

EMPTY = mr.EMPTY
MARGIN = 1e-4
ANGLE = 15.0


@pytest.fixture(scope="module")
def dev(ahv):
    return torch.device("cuda:0")


def make_case(ahv, N, B, per_sample, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, N)).astype(np.float32)
    R = ahv.rotations.haar_rotations_np(N * (B if per_sample else 1), seed + 1)
    return s, (R.reshape(B, N, 3, 3) if per_sample else R)


def run_modes(ahv, dev, s, R, K, angle=ANGLE, n_offset=0):
    """The kernel's list (B,K) on the CPU, and the reference's with its margin."""
    keys = ahv.ops.topk_modes(torch.from_numpy(s).to(dev), torch.from_numpy(np.ascontiguousarray(R)).to(dev), K, angle,
                              n_offset=n_offset)
    want, margin = mr.select_modes(s, R, K, angle, n_offset=n_offset)
    return keys.cpu(), torch.from_numpy(want), margin


# ---- shapes: tile edges, ragged 16-byte ends, several workgroups per sample ----------------------------------------
# (N, B, per-sample R, n_offset, K, seed).  N = 1023 / 1025 / 4097 / 20011 with a per-sample R: sample 1's row starts
# mid-vector (9 N floats is no multiple of 4), so the 16-byte path must key off the address.  K = 64 stays at the sizes
# where ~4e-6 * (decisions) leaves seeds with a 1e-4 margin: N * K * B decisions, all near-misses of tau counted.
SHAPES = [
    (1, 1, False, 0, 1, 0), (1, 3, True, 7, 8, 0), (1, 3, False, 0, 64, 0),
    (3, 1, False, 7, 8, 0), (3, 3, True, 0, 64, 0), (3, 3, False, 7, 1, 0),
    (1023, 1, False, 0, 64, 0), (1023, 3, True, 7, 8, 0), (1023, 3, False, 0, 1, 0), (1023, 3, True, 0, 64, 0),
    (1024, 1, False, 7, 8, 0), (1024, 3, False, 0, 64, 0), (1024, 3, True, 7, 1, 0),
    (1025, 1, False, 0, 1, 0), (1025, 3, True, 0, 64, 0), (1025, 3, False, 7, 8, 1),
    (4097, 1, False, 7, 64, 0), (4097, 3, True, 0, 8, 9), (4097, 3, False, 7, 8, 0), (4097, 3, True, 7, 1, 0),
    (20011, 1, False, 0, 8, 0), (20011, 3, True, 7, 8, 5), (20011, 3, False, 0, 1, 0), (20011, 3, False, 7, 8, 5),
]


@pytest.mark.parametrize("N,B,per_sample,n_offset,K,seed", SHAPES)
def test_list_equals_the_reference(ahv, dev, N, B, per_sample, n_offset, K, seed):
    s, R = make_case(ahv, N, B, per_sample, seed)
    got, want, margin = run_modes(ahv, dev, s, R, K, n_offset=n_offset)
    print("N=%d B=%d K=%d: margin %.3e" % (N, B, K, margin))
    assert margin >= MARGIN
    assert got.shape == (B, K) and got.dtype == torch.int64
    assert torch.equal(got, want)
    if K > N:
        assert bool((got[:, N:] == EMPTY).all())     # K > N: EMPTY padding
    # first entry = the arg-max key; the list is strictly descending up to the padding
    assert torch.equal(got[:, 0], ahv.ops.argmax(torch.from_numpy(s).to(dev), n_offset=n_offset, return_key=True).cpu())
    g = got.numpy()
    live = g != EMPTY
    assert np.all((g[:, 1:] < g[:, :-1]) | ~live[:, 1:]) and np.all(live[:, :-1] | ~live[:, 1:])


def test_caller_buffers_are_used_and_overwritten(ahv, dev):
    """``keys`` and ``workspace`` given: the list lands in ``keys`` whatever it held (no merge), nothing else is touched."""
    s, R = make_case(ahv, 1025, 3, False, 1)   # (the seed of the same shape in SHAPES: margin 5.2e-3)
    K = 8
    keys = torch.full((3, K), (1 << 62), dtype=torch.int64, device=dev)   # above every real key: a merge would keep it
    ws = ahv.ops.topk_modes_workspace(3, 1025, K, dev)
    assert ws.numel() * 8 == ahv._lib.load().ahv_topk_modes_workspace_bytes(3, 1025, K)
    out = ahv.ops.topk_modes(torch.from_numpy(s).to(dev), torch.from_numpy(R).to(dev), K, ANGLE, keys=keys, workspace=ws)
    want, margin = mr.select_modes(s, R, K, ANGLE)
    assert margin >= MARGIN and out.data_ptr() == keys.data_ptr() and torch.equal(keys.cpu(), torch.from_numpy(want))
    with pytest.raises(RuntimeError, match="workspace"):
        ahv.ops.topk_modes(torch.from_numpy(s).to(dev), torch.from_numpy(R).to(dev), K, ANGLE, workspace=ws[:100])


# ---- score content ----------------------------------------------------------------------------------------------------

def test_ties_specials_and_an_all_equal_row(ahv, dev):
    """Scores quantised to force ties (the lowest index wins), NaN of both signs, +-inf, +-0, and an all-equal row."""
    N, K = 2050, 16
    rng = np.random.default_rng(4)
    s = (np.round(rng.standard_normal((3, N)) * 4) / 4).astype(np.float32)       # ~25 distinct values
    s[1] = 0.75                                                                   # all equal: index order
    s[2] = -np.abs(s[2])                                                          # +-0 are the largest finite values
    p = rng.choice(N, 10, replace=False)
    s[0, p[0]], s[0, p[1]], s[0, p[2]], s[0, p[3]] = np.nan, np.inf, -np.inf, np.inf
    s[0].view(np.uint32)[p[4]] = 0xFFC00000                                       # NaN with the sign bit set
    s[2, p[5]], s[2, p[6]], s[2, p[7]], s[2, p[8]] = 0.0, -0.0, 0.0, -0.0
    R = ahv.rotations.haar_rotations_np(N, 9)
    got, want, margin = run_modes(ahv, dev, s, R, K, n_offset=3)
    assert margin >= MARGIN and torch.equal(got, want)
    idx = mr.indices(got.numpy()) - 3
    assert sorted(idx[0, :2].tolist()) == sorted([int(p[0]), int(p[4])]) and idx[0, 0] == min(p[0], p[4])   # the NaNs first
    assert idx[1, 0] == 0 and np.all(np.diff(idx[1]) > 0)                         # all equal: ascending indices
    assert len(np.unique(s[0, idx[0]][2:])) < K - 2                               # ties did reach the list


# ---- the clustered set: what the K-best list cannot do ----------------------------------------------------------------

def axis_angle(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def test_clustered_set_gives_one_mode_per_cluster(ahv, dev):
    """Five centres at least 40 degrees apart, 200 members within 3 degrees of each, random scores, shuffled: at 15 degrees and
    K = 8 the list is each cluster's best member, in score order, then three EMPTY entries -- while the K-best list spends
    several of its first five entries on one cluster.  Fails without the feature."""
    rng = np.random.default_rng(17)
    centres = [np.eye(3), axis_angle([1, 0, 0], 60), axis_angle([0, 1, 0], 75), axis_angle([0, 0, 1], 90), axis_angle([1, 1, 0], 150)]
    geo = lambda A, B: np.degrees(np.arccos(np.clip((np.sum(A * B) - 1) / 2, -1, 1)))
    assert min(geo(a, b) for i, a in enumerate(centres) for b in centres[:i]) >= 40.0
    R, cluster = [], []
    for c, C in enumerate(centres):
        for _ in range(200):
            R.append(C @ axis_angle(rng.standard_normal(3), rng.uniform(0, 3)))
            cluster.append(c)
    perm = rng.permutation(1000)
    R, cluster = np.asarray(R, dtype=np.float32)[perm], np.asarray(cluster)[perm]
    s = rng.standard_normal((1, 1000)).astype(np.float32)
    got, want, margin = run_modes(ahv, dev, s, R, 8)
    assert margin >= 0.05                                   # members <= 6 degrees apart, clusters >= 34: nothing near 15
    assert torch.equal(got, want)
    idx = mr.indices(got.numpy())[0]
    assert np.all(idx[5:] == -1) and np.all(idx[:5] >= 0)
    assert sorted(cluster[idx[:5]].tolist()) == [0, 1, 2, 3, 4]
    best = [int(np.flatnonzero(cluster == c)[np.argmax(s[0, cluster == c])]) for c in range(5)]
    assert idx[:5].tolist() == sorted(best, key=lambda i: -s[0, i])
    top = ahv.ops.select_topk(ahv.ops.topk(torch.from_numpy(s).to(dev), 8), torch.from_numpy(R).to(dev))[1].cpu().numpy()[0]
    assert len(set(cluster[top[:5]].tolist())) < 5          # the K-best list: one cluster several times


# ---- matrices that are no rotations -----------------------------------------------------------------------------------

def test_non_rotations_and_a_nan_matrix(ahv, dev):
    """Scaled, sheared, rank-deficient and zero matrices mixed into a Haar set: distinct indices (a winner whose |R|^2 is
    below tau still goes) and the reference's list.  A hypothesis with a NaN entry is neither suppressed nor suppresses."""
    Rm, names, _ = rotation_families.mixed(200, seed=7)
    R = np.concatenate([ahv.rotations.haar_rotations_np(1800, 12), Rm])
    R = R[np.random.default_rng(1).permutation(len(R))]
    N, K = len(R), 64
    s = np.random.default_rng(6).standard_normal((1, N)).astype(np.float32)
    order = np.argsort(-s[0], kind="stable")
    nan_i = int(order[1])                                   # the second best score gets the NaN matrix
    R[nan_i] = ahv.rotations.haar_rotations_np(1, 99)[0]
    R[nan_i, 1, 2] = np.nan
    got, want, margin = run_modes(ahv, dev, s, R, K)
    assert margin >= MARGIN and torch.equal(got, want)
    idx = mr.indices(got.numpy())[0]
    assert np.all(idx >= 0) and len(set(idx.tolist())) == K
    assert idx[0] == order[0] and idx[1] == nan_i           # not suppressed by the winner: t is NaN
    # and it suppressed nothing: without that hypothesis the rest of the list is the same
    s2 = s.copy()
    s2[0, nan_i] = -np.inf
    got2, want2, margin2 = run_modes(ahv, dev, s2, R, K - 1)
    assert margin2 >= MARGIN and torch.equal(got2, want2)
    assert mr.indices(got2.numpy())[0].tolist() == [i for i in idx.tolist() if i != nan_i]
    tau = float(mr.tau_of(ANGLE))
    assert np.sum(np.einsum("nab,nab->n", R[idx].astype(np.float64), R[idx].astype(np.float64)) < tau) >= 1


# ---- the committed fixtures through verify_pair_modes -----------------------------------------------------------------

@pytest.mark.parametrize("name,K,want_idx", [("score_n128", 7, [43, 1, 99, 18, 111, 85, 6]),
                                             ("score_n4096", 5, [2895, 2779, 1891, 2493, 3468])])
def test_fixture_modes(ahv, dev, g128, name, K, want_idx):
    g = load_golden(name)
    T = lambda k: torch.from_numpy(np.ascontiguousarray((g if k in g.files else g128)[k])).to(dev)   # n4096 holds R and scores only
    vs, vt, R, W1, W2, b2 = (T(k) for k in ("vol_src", "vol_tgt", "R", "W1", "W2", "b2"))
    keys = torch.empty((1, K), dtype=torch.int64, device=dev)
    m_s, m_i, m_R = ahv.ops.verify_pair_modes(vs, vt, R, W1, W2, b2, K, ANGLE, keys=keys)
    scores = ahv.ops.verify_pair(vs, vt, R, W1, W2, b2, want_scores=True)[0]
    want, margin = mr.select_modes(scores.cpu().numpy(), g["R"], K, ANGLE)
    assert margin >= MARGIN and torch.equal(keys.cpu(), torch.from_numpy(want))
    assert m_i.cpu().numpy()[0].tolist() == want_idx        # derived from the fixture's reference-run scores
    assert torch.equal(m_s, torch.gather(scores, 1, m_i)) and torch.equal(m_R, R[m_i])


# ---- CoarseToFine(modes=K) ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def step_inputs(ahv, dev, g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k])).to(dev)
    g = load_golden("batched")
    vs, vt = torch.from_numpy(g["vol_src"]).to(dev), torch.from_numpy(g["vol_tgt"]).to(dev)
    # Haar seed 43: the CPU oracle's coarse scores give a decision margin >= 2.4e-4 for all three samples in both input orders
    # (seed 40, the multi-seed test's, leaves 1.0e-5 for one of them: an input on which fp32 may not decide as fp64 does)
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(10_000, 43)).to(dev)
    return vs, vt, T("W1"), T("W2"), T("b2"), R


@pytest.mark.parametrize("B", [1, 3])
def test_mode_step_configs4_size(ahv, dev, step_inputs, B):
    """CoarseToFine(modes=4), 10 000 + 1 000, both input orders: eager, modes=1 against seeds=1, run_many."""
    vs3, vt3, W1, W2, b2, R = step_inputs
    vs, vt = vs3[:B].contiguous(), vt3[:B].contiguous()
    K, N2 = 4, 1000
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N2, max_angle_deg=10.0, batch=B, want_scores=True, **kw)
    eager, many = mk(modes=K, mode_angle_deg=ANGLE, use_graph=False), mk(modes=K, mode_angle_deg=ANGLE, use_graph=True)
    one_mode, one_seed = mk(modes=1, use_graph=False), mk(use_graph=False)
    Rn = R.cpu().numpy()
    results = []
    for rep in range(2):
        a, b = (vs, vt) if rep == 0 else (vt, vs)
        out = [t.clone() for t in eager(a, b)]
        score, idx, R_pred, c_score, c_idx = out
        s1, s2 = eager.last["coarse_scores"], eager.last["fine_scores"]
        top_s, top_i = eager.last["coarse_topk"]
        m_s, m_i, m_R = eager.last["modes"]
        # (i) the coarse modes = the reference on the step's own coarse scores
        want, margin = mr.select_modes(s1.cpu().numpy(), Rn, K, ANGLE)
        print("B=%d rep=%d: margin %.3e" % (B, rep, margin))
        assert margin >= MARGIN
        assert np.array_equal(top_i.cpu().numpy(), mr.indices(want)) and torch.equal(top_s, torch.gather(s1, 1, top_i))
        assert torch.equal(c_idx, top_i[:, 0]) and torch.equal(c_score, top_s[:, 0])
        # (ii) each mode's best refinement = the per-block torch.max of the fine scores; the winner = the best of those
        blocks = s2.view(B, K, N2)
        assert torch.equal(m_s, blocks.max(dim=2).values)
        assert torch.equal(torch.gather(blocks, 2, m_i[:, :, None])[:, :, 0], m_s) and bool(((0 <= m_i) & (m_i < N2)).all())
        first = (blocks == m_s[:, :, None]).to(torch.int64).argmax(dim=2)      # lowest index among equal scores
        assert torch.equal(m_i, first)
        R_fine = eager.last["R_fine"].view(B, K, N2, 3, 3)
        ar = torch.arange(B, device=dev)
        assert torch.equal(m_R, R_fine[ar[:, None], torch.arange(K, device=dev)[None], m_i])
        best = m_s.argmax(dim=1)
        assert torch.equal(score, m_s[ar, best]) and torch.equal(idx, best * N2 + m_i[ar, best])
        assert torch.equal(R_pred, m_R[ar, best])
        # (iii) modes = 1 is the seeds = 1 step, bit for bit
        for x, y in zip(one_mode(a, b), one_seed(a, b)):
            assert torch.equal(x, y)
        assert torch.equal(one_mode.last["fine_scores"], one_seed.last["fine_scores"])
        results.append(out)
    # (iv) a run_many graph of 3 steps = three eager steps (the second round replays the captured graph)
    vsm, vtm = torch.stack([vs, vt, vs]), torch.stack([vt, vs, vt])
    for rnd in range(2):
        outs = many.run_many(vsm, vtm, steps=3)
        for k in range(3):
            for x, y in zip(outs[k], results[k % 2]):
                assert torch.equal(x, y), (rnd, k)


def test_mode_step_with_polishing(ahv, dev, step_inputs):
    """``polish_iters > 0``: all K per-mode poses are polished, none scores below its start, the best polished one is returned."""
    vs3, vt3, W1, W2, b2, R = step_inputs
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=1000, batch=3, modes=4, mode_angle_deg=ANGLE, polish_iters=2,
                                  use_graph=False)
    score, idx, R_pred, _, _ = c2f(vs3, vt3)
    p, (m_s, m_i, m_R) = c2f.last["polish"], c2f.last["modes"]
    assert p["score_after"].shape == (3, 4) and torch.equal(p["score_before"], m_s) and torch.equal(p["R_before"], m_R)
    assert bool((p["score_after"] >= m_s).all())
    best = p["score_after"].argmax(dim=1)
    ar = torch.arange(3, device=dev)
    assert torch.equal(score, p["score_after"][ar, best]) and torch.equal(R_pred, p["R_after"][ar, best])
    assert torch.equal(idx, best * 1000 + m_i[ar, best])


RANK_WORKER = r'''
import importlib, os, sys, numpy as np, torch
import torch.distributed as dist
sys.path.insert(0, os.environ["AHV_REPO"])
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
ahv = importlib.import_module("3dahv_amd")
g = np.load(os.path.join(os.environ["AHV_REPO"], "tests", "golden", "batched.npz"))
h = np.load(os.path.join(os.environ["AHV_REPO"], "tests", "golden", "score_n128.npz"))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
vs, vt, W1, W2, b2 = T(g["vol_src"]), T(g["vol_tgt"]), T(h["W1"]), T(h["W2"]), T(h["b2"])
R = torch.from_numpy(ahv.rotations.haar_rotations_np(10_000, 43)).to(dev)
calls = []
real_reduce, real_gather = dist.all_reduce, dist.all_gather_into_tensor
dist.all_reduce = lambda t, *a, **k: (calls.append(("all_reduce", tuple(t.shape))), real_reduce(t, *a, **k))[1]
dist.all_gather_into_tensor = lambda o, t, *a, **k: (calls.append(("all_gather", tuple(t.shape))), real_gather(o, t, *a, **k))[1]
mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=1000, batch=3, modes=4, mode_angle_deg=15.0, want_scores=True, **kw)
forced, forced_eager, plain = mk(force_collectives=True), mk(force_collectives=True, use_graph=False), mk(use_graph=False)
assert forced.collectives and forced.use_graph and forced_eager.collectives and not plain.collectives
for rep in range(3):
    a, b = (vs, vt) if rep != 1 else (vt, vs)
    ref = [t.clone() for t in plain(a, b)]
    n0 = len(calls)
    for x, y in zip([t.clone() for t in forced_eager(a, b)], ref):
        assert torch.equal(x, y), (rep, x, y)
    assert calls[n0:] == [("all_gather", (3, 10_000)), ("all_reduce", (3, 4))], calls[n0:]   # two collectives per step
    for x, y in zip([t.clone() for t in forced(a, b)], ref):
        assert torch.equal(x, y), (rep, x, y)
    for name in ("coarse_topk", "modes"):
        assert all(torch.equal(x, y) for x, y in zip(forced.last[name], plain.last[name])), name
    assert torch.equal(forced.last["fine_scores"], plain.last["fine_scores"])
    assert torch.equal(forced.last["coarse_scores"], plain.last["coarse_scores"])
torch.cuda.synchronize()
print("OK graph=%s" % forced.use_graph)
dist.destroy_process_group()
'''


def test_mode_step_with_rccl_collectives_captured(tmp_path):
    """A 1-rank RCCL group with the collectives forced, in a process of its own: the score all-gather, the selection over the
    gathered row and the (B,K) key all-reduce are captured into the step's hipGraph; results equal the plain step's."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "modes_worker.py"
    script.write_text(RANK_WORKER)
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AHV_REPO=REPO,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout
    assert "OK graph=True" in p.stdout, p.stdout
