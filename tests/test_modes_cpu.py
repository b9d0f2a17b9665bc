"""Distinct pose modes, CPU tier: argument validation of ``ahv_topk_modes_f32`` / ``ahv_topk_modes_workspace_bytes`` through
the ctypes table (validation runs before any HIP call), the properties of the numpy reference (tests/modes_reference.py), and
``CoarseToFine(modes=K)``'s control flow on an oracle-backed CPU backend -- world 1, and world 2 under gloo against world 1
(same coarse modes, same per-mode results, same winner, bit for bit)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import modes_reference as mr
from . import rotation_families
from .conftest import REPO, load_golden
from .test_dist_cpu import _free_port
from .test_refine_dist_cpu import _inputs as _inputs96
from .test_topk_cpu import TopkOracleBackend

# 95 coarse hypotheses and 3 blocks of 40: two ranks get uneven coarse shards (47 + 48) and cut the middle block in half
N_COARSE, N_FINE, MODES, ANGLE = 95, 40, 3, 40.0


def _inputs(ahv):
    vs, vt, W1, W2, b2, _ = _inputs96(ahv)
    return vs, vt, W1, W2, b2, torch.from_numpy(ahv.rotations.haar_rotations_np(N_COARSE, seed=21))


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


class ModesOracleBackend(TopkOracleBackend):
    """The CPU backend protocol with the two operations ``modes=K`` adds: the numpy reference and a host arg-max key."""

    def topk_modes(self, scores, R, k, min_angle_deg, n_offset=0, keys=None, workspace=None):
        new = torch.from_numpy(mr.select_modes(scores.numpy(), R.numpy(), k, min_angle_deg, n_offset)[0])
        if keys is None:
            return new
        keys.copy_(new)
        return keys

    def argmax(self, scores, n_offset=0, return_key=False):
        assert return_key
        s = scores.numpy()
        idx = np.broadcast_to(np.arange(s.shape[1], dtype=np.int64) + n_offset, s.shape)
        return torch.from_numpy(self.ahv.dist.pack_keys_host(s, idx).reshape(s.shape).max(axis=1))


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------

def test_modes_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    ws_bytes = lib.ahv_topk_modes_workspace_bytes
    # a pure function of (B, N, K): one packed key per sample and hypothesis, N rounded up to a lane's four
    assert ws_bytes(0, 50_000, 8) == 0 and ws_bytes(3, 0, 8) == 0
    assert ws_bytes(3, 50_000, 0) == 0 and ws_bytes(3, 50_000, 65) == 0
    assert ws_bytes(1, 50_000, 8) == 8 * 50_000 == ws_bytes(1, 50_000, 64)
    assert ws_bytes(3, 1023, 8) == 8 * 3 * 1024 and ws_bytes(3, 1025, 1) == 8 * 3 * 1028 and ws_bytes(1, 1, 1) == 32

    tau = float(mr.tau_of(15.0))
    # (scores, R, r_batch_stride, B, N, n_offset, K, min_trace, keys, workspace, workspace_bytes, stream)
    modes = lib.ahv_topk_modes_f32
    big = 1 << 20
    for bad in (0, 65, -1):
        assert modes(1, 1, 0, 1, 10, 0, bad, tau, 1, 16, big, None) == -1 and b"K" in err() and str(bad).encode() in err()
    for bad in (-1.0, 3.0, float("nan"), float("inf"), -float("inf"), 3.5, -1.5):
        assert modes(1, 1, 0, 1, 10, 0, 4, bad, 1, 16, big, None) == -1 and b"min_trace" in err(), bad
    assert modes(None, 1, 0, 1, 10, 0, 4, tau, 1, 16, big, None) == -1 and b"null" in err()
    assert modes(1, None, 0, 1, 10, 0, 4, tau, 1, 16, big, None) == -1 and b"null" in err()
    assert modes(1, 1, 0, 1, 10, 0, 4, tau, None, 16, big, None) == -1 and b"null" in err()
    assert modes(1, 1, 0, 1, -10, 0, 4, tau, 1, 16, big, None) == -1 and b"negative" in err()
    assert modes(1, 1, 0, -1, 10, 0, 4, tau, 1, 16, big, None) == -1 and b"negative" in err()
    assert modes(1, 1, 0, 65536, 10, 0, 4, tau, 1, 16, big, None) == -1 and b"65535" in err()
    assert modes(1, 1, 0, 1, 10, 1 << 32, 4, tau, 1, 16, big, None) == -1 and b"32 bits" in err()
    for bad in (5, 89, 91, -90):
        assert modes(1, 1, bad, 1, 10, 0, 4, tau, 1, 16, big, None) == -1 and b"r_batch_stride" in err()
    assert modes(1, 1, 0, 1, 10, 0, 4, tau, 1, None, 0, None) == -1 and b"workspace" in err()
    assert modes(1, 1, 0, 1, 10, 0, 4, tau, 1, 16, 8 * 12 - 1, None) == -1 and b"workspace" in err()
    assert modes(1, 1, 0, 1, 10, 0, 4, tau, 1, 24, big, None) == -1 and b"aligned" in err()
    assert modes(None, None, 0, 0, 10, 0, 4, tau, None, None, 0, None) == 0   # B = 0: nothing to do
    assert lib.ahv_abi_version() == (2 << 16) | 3   # added under 2.3: callers probe for the symbol


def test_modes_ops_refuse_cpu_tensors(ahv):
    R = torch.eye(3)[None].repeat(8, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.topk_modes(torch.zeros(2, 8), R, 4, 15.0)
    with pytest.raises(RuntimeError, match="K = 65"):
        ahv.ops.topk_modes(torch.zeros(2, 8), R, 65, 15.0)
    for bad in (0.0, 180.0, -5.0, 1e-6, float("nan")):   # 1e-6 degrees: 1 + 2 cos rounds to 3 in fp32
        with pytest.raises(RuntimeError, match="min_angle_deg"):
            ahv.ops.topk_modes(torch.zeros(2, 8), R, 4, bad)
    assert ahv.ops.min_trace(15.0) == float(mr.tau_of(15.0))


# ---- the reference's own properties ---------------------------------------------------------------------------

def test_reference_is_a_subsequence_of_the_stable_sort(ahv):
    rng = np.random.default_rng(11)
    B, N, K = 3, 700, 16
    s = rng.standard_normal((B, N)).astype(np.float32)
    s[:, rng.integers(0, N, 100)] = s[:, rng.integers(0, N, 100)]   # ties
    s[0, 5], s[1, 9], s[2, 17] = np.nan, np.inf, -np.inf
    R = ahv.rotations.haar_rotations_np(N, 3)
    keys, margin = mr.select_modes(s, R, K, 25.0, n_offset=7)
    assert margin > 0
    idx = mr.indices(keys) - 7
    order = torch.sort(torch.from_numpy(s), dim=1, descending=True, stable=True).indices.numpy()
    tau = float(mr.tau_of(25.0))
    for b in range(B):
        got = idx[b][keys[b] != mr.EMPTY]
        pos = [int(np.flatnonzero(order[b] == i)[0]) for i in got]
        assert pos == sorted(pos) and len(set(pos)) == len(pos) and pos[0] == 0   # a subsequence, the arg-max first
        # pairwise separated, and every hypothesis ranked above the last entry is within theta of an earlier entry
        t = np.einsum("iab,jab->ij", R[got].astype(np.float64), R[got].astype(np.float64))
        assert np.all(t[~np.eye(len(got), dtype=bool)] < tau)
        for p in range(pos[-1]):
            i = order[b][p]
            if i in got:
                continue
            earlier = [g for g, q in zip(got, pos) if q < p]
            assert max(float(np.sum(R[i].astype(np.float64) * R[g])) for g in earlier) >= tau
    k1, _ = mr.select_modes(s, R, 1, 25.0, n_offset=7)
    assert np.array_equal(k1[:, 0], ahv.dist.pack_keys_host(s, np.arange(N) + 7).reshape(B, N).max(axis=1))   # K = 1: the arg-max


def test_reference_never_repeats_a_winner_for_non_rotations(ahv):
    """t(w, w) = |R_w|^2 is below tau for zero, shrunk and rank-deficient matrices: the winner still goes, by its index."""
    Ro, names = rotation_families.outside(64, seed=3)
    R = np.concatenate([Ro, np.zeros((4, 3, 3), np.float32), 0.3 * ahv.rotations.haar_rotations_np(12, 5)])
    N = len(R)
    tau = float(mr.tau_of(15.0))
    assert np.sum(np.einsum("nab,nab->n", R.astype(np.float64), R.astype(np.float64)) < tau) >= 20
    s = np.random.default_rng(2).standard_normal((2, N)).astype(np.float32)
    keys, _ = mr.select_modes(s, R, 64, 15.0)
    idx = mr.indices(keys)
    for b in range(2):
        got = idx[b][idx[b] >= 0]
        assert len(set(got.tolist())) == len(got) and len(got) >= 20
    # all-zero matrices: nothing is ever suppressed, the list is the K-best list
    kz, _ = mr.select_modes(s, np.zeros((N, 3, 3), np.float32), 10, 15.0)
    order = torch.sort(torch.from_numpy(s), dim=1, descending=True, stable=True).indices.numpy()[:, :10]
    assert np.array_equal(mr.indices(kz), order)
    # K beyond the number of modes: EMPTY padding (identical rotations: one mode)
    ke, _ = mr.select_modes(s, np.broadcast_to(np.eye(3, dtype=np.float32), (N, 3, 3)), 5, 15.0)
    assert np.all(ke[:, 1:] == mr.EMPTY) and np.array_equal(mr.indices(ke)[:, 0], order[:, 0])


def test_fixture_lists_rederived(ahv):
    """The lists of the two committed fixtures at 15 degrees, from their reference-run scores (tests/test_gpu_modes.py pins
    the kernel to the same indices)."""
    for name, K, want in (("score_n128", 7, [43, 1, 99, 18, 111, 85, 6]), ("score_n4096", 5, [2895, 2779, 1891, 2493, 3468])):
        g = load_golden(name)
        keys, margin = mr.select_modes(g["scores"], g["R"], K, 15.0)
        assert mr.indices(keys)[0].tolist() == want and margin >= 2.4e-3


# ---- CoarseToFine(modes=K) on the CPU backend ---------------------------------------------------------------

def _run(ahv, oracle, modes=MODES, **extra):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3, use_graph=True,
                                  backend=ModesOracleBackend(ahv, oracle), want_scores=True, modes=modes,
                                  mode_angle_deg=ANGLE, **extra)
    assert not c2f.use_graph  # CPU tensors / gloo: eager
    out = [t.clone().numpy() for t in c2f(vs, vt)]
    return c2f, out


def test_modes_argument_is_checked(ahv, oracle):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, backend=ModesOracleBackend(ahv, oracle), **kw)
    with pytest.raises(RuntimeError, match="seeds"):
        mk(modes=4, seeds=2)
    with pytest.raises(RuntimeError, match="fused"):
        ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, fused=True, modes=4)
    for bad in (65, -1):
        with pytest.raises(RuntimeError, match="modes"):
            mk(modes=bad)
    for bad in (0.0, 180.0):
        with pytest.raises(RuntimeError, match="min_angle_deg"):
            mk(modes=4, mode_angle_deg=bad)
    assert mk().modes == 0 and mk(modes=4).seeds == 4 and mk(modes=4).modes == 4


def test_mode_step_world1(ahv, oracle):
    c2f, out = _run(ahv, oracle)
    score, idx, R_pred, c_score, c_idx = out
    one = ahv.refine.CoarseToFine(*_inputs(ahv)[2:], n_fine=N_FINE, max_angle_deg=12.0, batch=3,
                                  backend=ModesOracleBackend(ahv, oracle), want_scores=True)
    ref1 = [t.clone().numpy() for t in one(*_inputs(ahv)[:2])]
    s1 = c2f.last["coarse_scores"].numpy()
    top_s, top_i = (t.numpy() for t in c2f.last["coarse_topk"])
    m_s, m_i, m_R = (t.numpy() for t in c2f.last["modes"])
    want_keys, margin = mr.select_modes(s1, c2f.R_coarse.numpy(), MODES, ANGLE)
    assert margin >= 1e-4
    assert np.array_equal(top_i, mr.indices(want_keys)) and np.all(top_i >= 0)
    assert np.array_equal(top_s, np.take_along_axis(s1, top_i, axis=1))
    # the modes are not the largest scores: the feature does something on this input
    order = torch.sort(torch.from_numpy(s1), dim=1, descending=True, stable=True).indices.numpy()[:, :MODES]
    assert not np.array_equal(top_i, order)
    assert np.array_equal(c_idx, ref1[4]) and np.array_equal(c_score, ref1[3])   # first entry = the arg-max
    Rf = c2f.last["R_fine"].numpy()
    want_Rf = torch.matmul(c2f.R_coarse[torch.from_numpy(top_i)][:, :, None], c2f.D[None, None]).reshape(3, -1, 3, 3)
    assert np.array_equal(Rf, want_Rf.numpy())
    s2 = c2f.last["fine_scores"].numpy().reshape(3, MODES, N_FINE)
    assert np.array_equal(m_s, s2.max(axis=2)) and np.array_equal(m_i, s2.argmax(axis=2))
    assert np.array_equal(m_R, Rf.reshape(3, MODES, N_FINE, 3, 3)[np.arange(3)[:, None], np.arange(MODES)[None], m_i])
    best = m_s.argmax(axis=1)
    assert np.array_equal(score, m_s.max(axis=1)) and np.array_equal(idx, best * N_FINE + m_i[np.arange(3), best])
    assert np.array_equal(R_pred, m_R[np.arange(3), best])
    again = [t.clone().numpy() for t in c2f(*_inputs(ahv)[:2])]
    for a, b in zip(again, out):
        assert np.array_equal(a, b)


def test_modes_one_is_the_single_seed_step(ahv, oracle):
    a, out_a = _run(ahv, oracle, modes=1)
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    b = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3,
                                backend=ModesOracleBackend(ahv, oracle), want_scores=True)
    out_b = [t.clone().numpy() for t in b(vs, vt)]
    for x, y in zip(out_a, out_b):
        assert np.array_equal(x, y)
    assert np.array_equal(a.last["fine_scores"].numpy(), b.last["fine_scores"].numpy())
    assert np.array_equal(a.last["modes"][0].numpy()[:, 0], out_b[0])


def test_an_empty_mode_takes_no_part(ahv, oracle):
    """More modes asked for than the set holds (160 degrees: at most a handful): the list ends EMPTY, the per-mode entries of
    those slots are (-inf, -1, zeros) and the winner comes from a real mode although the EMPTY slots' blocks were scored."""
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    K = 12
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3,
                                  backend=ModesOracleBackend(ahv, oracle), want_scores=True, modes=K, mode_angle_deg=160.0)
    score, idx, R_pred, _, _ = [t.clone().numpy() for t in c2f(vs, vt)]
    top_s, top_i = (t.numpy() for t in c2f.last["coarse_topk"])
    m_s, m_i, m_R = (t.numpy() for t in c2f.last["modes"])
    empty = top_i < 0
    assert empty.any(axis=1).all() and not empty[:, 0].any()
    assert np.all(m_s[empty] == -np.inf) and np.all(m_i[empty] == -1) and np.all(m_R[empty] == 0)
    s2 = c2f.last["fine_scores"].numpy().reshape(3, K, N_FINE)
    assert np.array_equal(m_s[~empty], s2.max(axis=2)[~empty])
    assert np.array_equal(score, m_s.max(axis=1)) and np.all(idx // N_FINE < (~empty).sum(axis=1))


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
        real_reduce, real_gather = dist.all_reduce, dist.all_gather_into_tensor
        dist.all_reduce = lambda t, *a, **k: (calls.append(("all_reduce", tuple(t.shape))), real_reduce(t, *a, **k))[1]
        dist.all_gather_into_tensor = lambda o, t, *a, **k: (calls.append(("all_gather", tuple(t.shape))),
                                                             real_gather(o, t, *a, **k))[1]
        try:
            c2f, out = _run(ahv, oracle)
        finally:
            dist.all_reduce, dist.all_gather_into_tensor = real_reduce, real_gather
        assert c2f.world == world and c2f.collectives
        # still TWO exchanges per step: the coarse-score gather, then the (B,K) per-block keys
        assert calls == [("all_gather", (3, -(-N_COARSE // world))), ("all_reduce", (3, MODES))], calls
        q.put((rank, (c2f.c_lo, c2f.c_hi, c2f.f_lo, c2f.f_hi), out, [t.numpy() for t in c2f.last["coarse_topk"]],
               [t.numpy() for t in c2f.last["modes"]], c2f.last["coarse_scores"].numpy(), c2f.last["fine_scores"].numpy()))
    finally:
        dist.destroy_process_group()


def test_mode_step_world2_equals_single_rank(ahv, oracle):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    single, ref = _run(ahv, oracle)
    ref_top = [t.numpy() for t in single.last["coarse_topk"]]
    ref_modes = [t.numpy() for t in single.last["modes"]]
    names = ["fine score", "fine index", "R_pred", "coarse score", "coarse index"]
    for rank, (c_lo, c_hi, f_lo, f_hi), out, top, modes, s1, s2 in got:
        for name, a, b in zip(names, out, ref):
            assert np.array_equal(a, b), (rank, name)
        assert all(np.array_equal(a, b) for a, b in zip(top, ref_top)), rank      # the same coarse modes
        assert all(np.array_equal(a, b) for a, b in zip(modes, ref_modes)), rank  # the same per-mode results
        assert (f_lo, f_hi) == ahv.dist.shard_range(MODES * N_FINE, rank, world)
        assert np.array_equal(s1, single.last["coarse_scores"].numpy())           # the gathered row is the whole row
        assert np.array_equal(s2, single.last["fine_scores"].numpy()[:, f_lo:f_hi])


def test_all_gather_scores_without_a_group_returns_the_slice(ahv):
    s = torch.arange(12.0).reshape(2, 6)
    assert ahv.dist.all_gather_scores(s, 6) is s
    with pytest.raises(ValueError, match="expected 7"):
        ahv.dist.all_gather_scores(s, 7)
