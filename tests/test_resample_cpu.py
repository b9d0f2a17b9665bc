"""Posterior resampling, CPU tier: the properties of the numpy reference (tests/resample_reference.py), argument validation of
``ahv_resample_f32`` / ``ahv_compose_rotations_indexed_f32`` through the ctypes table (validation runs before any HIP call),
the host-side checks of the ops, and ``CoarseToFine(resample=True)``'s control flow on an oracle-backed CPU backend -- world 1,
and world 2 under gloo against world 1 (same draw list, same winner, bit for bit)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import resample_reference as rr
from .conftest import REPO
from .test_dist_cpu import _free_port
from .test_refine_dist_cpu import _inputs as _inputs96
from .test_topk_cpu import TopkOracleBackend

# 95 coarse hypotheses and 41 draws: two ranks get uneven shards of both (47 + 48 coarse, 20 + 21 fine)
N_COARSE, N_FINE, TEMP, U = 95, 41, 0.05, 0.25


def _inputs(ahv):
    vs, vt, W1, W2, b2, _ = _inputs96(ahv)
    return vs, vt, W1, W2, b2, torch.from_numpy(ahv.rotations.haar_rotations_np(N_COARSE, seed=21))


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


class ResampleOracleBackend(TopkOracleBackend):
    """The CPU backend protocol with the three operations ``resample=True`` adds: the numpy reference and a host arg-max key."""

    def resample(self, scores, m, temperature=0.1, u=None, out=None, workspace=None):
        new = torch.from_numpy(rr.resample(scores.numpy(), m, temperature, None if u is None else u.numpy()))
        if out is None:
            return new
        out.copy_(new)
        return out

    def compose_rotations_indexed(self, idx, R, D, out=None):
        r = torch.from_numpy(rr.compose_rotations_indexed(idx.numpy(), R.numpy(), D.numpy()))
        if out is None:
            return r
        out.copy_(r)
        return out

    def argmax(self, scores, n_offset=0, return_key=False):
        assert return_key
        s = scores.numpy()
        idx = np.broadcast_to(np.arange(s.shape[1], dtype=np.int64) + n_offset, s.shape)
        return torch.from_numpy(self.ahv.dist.pack_keys_host(s, idx).reshape(s.shape).max(axis=1))


def _rows(seed=0):
    """Rows with every special value: (name, scores (N,), temperature)."""
    rng = np.random.default_rng(seed)
    out = []
    for N in (1, 3, 257, 1025):
        s = rng.uniform(-0.2, 0.6, N).astype(np.float32)
        out.append(("uniform%d" % N, s, 0.1))
        out.append(("sharp%d" % N, s, 0.02))
    s = rng.uniform(-0.2, 0.6, 300).astype(np.float32)
    s[[0, 7, 150, 299]] = [np.nan, np.inf, -np.inf, np.nan]
    out.append(("holes", s, 0.1))
    out.append(("equal", np.full(40, 0.25, np.float32), 0.1))
    peaked = np.full(500, -0.9, np.float32)
    peaked[123] = 0.9
    out.append(("peaked", peaked, 0.02))
    return out


# ---- the reference's own properties ---------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 7, 64, 1000])
def test_reference_partitions_the_slots(M):
    for name, s, T in _rows():
        beta = rr.beta_of(T)
        for u in (None, 0.0, 0.25, np.nextafter(np.float32(1), np.float32(0))):
            idx = rr.resample_row(s, beta, M, u)
            assert idx.shape == (M,) and idx.dtype == np.int64, name       # every slot once: the list has M entries
            fig = rr.check_draws(idx, s, beta, u)                          # non-decreasing, inside the scored set, to eps
            assert fig["cdf_miss"] <= 1e-15, (name, fig)                   # (the reference sits inside its own intervals)
            # floor(M p) / ceil(M p) copies of every hypothesis
            p, _, _ = rr.cdf(s, beta)
            count = np.bincount(idx, minlength=len(s))
            mp_ = M * p.astype(np.longdouble)
            assert np.all(count >= np.floor(mp_ - 1e-9)) and np.all(count <= np.ceil(mp_ + 1e-9)), name
            assert count.sum() == M


def test_reference_agrees_with_searchsorted_and_with_the_boundary_form():
    """Two statements of one rule: the draw's position looked up in the CDF (np.searchsorted, fp64 here) and the slots
    [h_{i-1}, h_i) each hypothesis owns.  fp64 against longdouble may move a draw that sits within 1e-13 of a boundary: none
    of these rows has one."""
    for name, s, T in _rows(seed=5):
        beta = rr.beta_of(T)
        for M in (5, 64, 1000):
            for u in (0.5, 0.125):
                a = rr.resample_row(s, beta, M, u)
                b = rr.resample_row_by_boundaries(s, beta, M, u)
                assert np.array_equal(a, b), (name, M, u)
                w, _ = rr.weights(s, beta)
                C = np.cumsum(w)
                t = (np.arange(M) + u) * C[-1] / M
                gap = np.abs(C[None, :] - t[:, None]).min() / C[-1]
                c = np.searchsorted(C, t, side="right")
                assert gap < 1e-13 or np.array_equal(a, c), (name, M, u, gap)


def test_reference_special_cases():
    beta = rr.beta_of(0.1)
    assert np.all(rr.resample_row(np.array([np.nan, np.inf, -np.inf], np.float32), beta, 9) == -1)
    # equal scores: weights of exactly 1, draw j is hypothesis floor((j + u) N / M)
    s = np.full(8, 0.3, np.float32)
    assert np.array_equal(rr.resample_row(s, beta, 16, 0.5), np.arange(16) // 2)
    assert np.array_equal(rr.resample_row(s, beta, 4, 0.0), [0, 2, 4, 6])
    assert np.array_equal(rr.resample_row(s, beta, 4, 0.5), [1, 3, 5, 7])
    # an offset outside [0, 1), NaN included, counts as 0.5
    for bad in (1.0, 1.5, -0.1, np.nan):
        assert np.array_equal(rr.resample_row(s, beta, 4, bad), [1, 3, 5, 7])
    # holes are never drawn
    s[[0, 3]] = [np.nan, -np.inf]
    assert np.array_equal(rr.resample_row(s, beta, 6, 0.5), [1, 2, 4, 5, 6, 7])
    # one peak takes every draw
    p = np.full(100, -0.9, np.float32)
    p[37] = 0.9
    assert np.all(rr.resample_row(p, rr.beta_of(0.02), 5000) == 37)
    assert abs(rr.tolerance(np.array([-0.2, 0.6], np.float32), beta) - 2.4e-6) < 1e-7


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------

def test_resample_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    wb = lib.ahv_resample_workspace_bytes
    # a pure function of (B, N): per sample a 32-byte header and one 16-byte record per tile of 1024, plus one
    assert wb(1, 1) == 32 + 2 * 16 and wb(1, 1024) == 64 and wb(1, 1025) == 32 + 3 * 16 and wb(3, 4099) == 3 * (32 + 6 * 16)
    assert wb(1, 10_000) == 32 + 11 * 16 and wb(1, 50_000) % 16 == 0
    assert wb(0, 10) == 0 and wb(-1, 10) == 0 and wb(1, 0) == 0 and wb(1, (1 << 32) + 1) == 0
    big = 1 << 20
    # (scores, B, N, beta, M, u, idx, workspace, workspace_bytes, flags, stream)
    rs = lib.ahv_resample_f32
    assert rs(16, -1, 10, 10.0, 5, None, 16, 16, big, 0, None) == -1 and b"negative" in err()
    assert rs(16, 65536, 10, 10.0, 5, None, 16, 16, big, 0, None) == -1 and b"65535" in err()
    for bad in (0, -3, (1 << 32) + 1):
        assert rs(16, 1, bad, 10.0, 5, None, 16, 16, big, 0, None) == -1 and b"N = " in err(), bad
    for bad in (0, -1, 1 << 31):
        assert rs(16, 1, 10, 10.0, bad, None, 16, 16, big, 0, None) == -1 and b"M = " in err(), bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rs(16, 1, 10, bad, 5, None, 16, 16, big, 0, None) == -1 and b"beta" in err(), bad
    assert rs(16, 1, 10, 10.0, 5, None, 16, 16, big, 1, None) == -1 and b"flags" in err()
    assert rs(None, 1, 10, 10.0, 5, None, 16, 16, big, 0, None) == -1 and b"null" in err()
    assert rs(16, 1, 10, 10.0, 5, None, None, 16, big, 0, None) == -1 and b"null" in err()
    assert rs(16, 1, 10, 10.0, 5, None, 16, None, 0, 0, None) == -1 and b"workspace" in err()
    assert rs(16, 1, 10, 10.0, 5, None, 16, 16, wb(1, 10) - 1, 0, None) == -1 and b"workspace" in err()
    assert rs(16, 1, 10, 10.0, 5, None, 16, 24, big, 0, None) == -1 and b"aligned" in err()
    assert rs(None, 0, 10, 10.0, 5, None, None, None, 0, 0, None) == 0          # B = 0: nothing to do
    # (idx, R, r_batch_stride, N, D, M, B, out, stream)
    ci = lib.ahv_compose_rotations_indexed_f32
    assert ci(16, 16, 0, 10, 16, -1, 1, 16, None) == -1 and b"negative" in err()
    assert ci(16, 16, 0, -10, 16, 5, 1, 16, None) == -1 and b"negative" in err()
    assert ci(16, 16, 0, 10, 16, 5, -1, 16, None) == -1 and b"negative" in err()
    for bad in (5, 89, 91, -90):
        assert ci(16, 16, bad, 10, 16, 5, 1, 16, None) == -1 and b"r_batch_stride" in err()
    for k in range(4):
        a = [16, 16, 0, 10, 16, 5, 1, 16, None]
        a[(0, 1, 4, 7)[k]] = None
        assert ci(*a) == -1 and b"null" in err()
    assert ci(16, 16, 0, 0, 16, 5, 1, 16, None) == -1 and b"empty rotation set" in err()
    assert ci(16, 16, 0, 10, 16, 1 << 30, 1 << 15, 16, None) == -1 and b"2^38" in err()
    assert ci(None, None, 0, 10, None, 5, 0, None, None) == 0 and ci(None, None, 0, 10, None, 0, 1, None, None) == 0
    assert lib.ahv_abi_version() == (2 << 16) | 3   # added under 2.3: callers probe for the symbol


def test_header_and_ctypes_table_agree_on_the_new_prototypes(ahv):
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ahv.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
             "unsigned": ctypes.c_uint}
    for name in ("ahv_resample_workspace_bytes", "ahv_resample_f32", "ahv_compose_rotations_indexed_f32"):
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        want_args = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (x.strip() for x in m.group(2).split(","))]
        res, args = ahv._lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and args == want_args, name


# ---- host checks ----------------------------------------------------------------------------------------------

def test_ops_check_arguments_before_any_launch(ahv):
    s, R = torch.zeros(2, 8), torch.eye(3)[None].repeat(8, 1, 1)
    D = torch.eye(3)[None].repeat(5, 1, 1)
    idx = torch.zeros(2, 5, dtype=torch.int64)
    rs, ci = ahv.ops.resample, ahv.ops.compose_rotations_indexed
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs(s, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs(s, 5, u=torch.zeros(2))
    for bad in (0, -1, 1 << 31):
        with pytest.raises(RuntimeError, match="draws"):
            rs(s, bad)
    for bad in (0.0, -0.1, float("nan"), float("inf"), 1e-45):
        with pytest.raises(RuntimeError, match="temperature"):
            rs(s, 5, bad)
    with pytest.raises(RuntimeError, match=r"\(B,N\)"):
        rs(torch.zeros(8), 5)
    with pytest.raises(RuntimeError, match="N = 0"):
        rs(torch.zeros(2, 0), 5)
    for bad in (torch.zeros(3), torch.zeros(2, 1), torch.zeros(2, dtype=torch.float64), 0.5):
        with pytest.raises(RuntimeError, match="u must be"):
            rs(s, 5, u=bad)
    for bad in (torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="out must be"):
            rs(s, 5, out=bad)
    with pytest.raises(RuntimeError, match="workspace of 16 bytes"):
        rs(s, 5, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ci(idx, R, D)
    with pytest.raises(RuntimeError, match="idx must be"):
        ci(idx.to(torch.int32), R, D)
    with pytest.raises(RuntimeError, match="idx must be"):
        ci(idx[0], R, D)
    with pytest.raises(RuntimeError, match="draws"):
        ahv.ops.verify_pair_resampled(None, None, R, torch.zeros(0, 3, 3), None, None, None)
    with pytest.raises(RuntimeError, match="temperature"):
        ahv.ops.verify_pair_resampled(None, None, R, D, None, None, None, temperature=0.0)
    with pytest.raises(RuntimeError, match=r"\(M,3,3\)"):
        ahv.ops.verify_pair_resampled(None, None, R, torch.zeros(5, 9), None, None, None)


# ---- CoarseToFine(resample=True) on the CPU backend ----------------------------------------------------------

def _run(ahv, oracle, **extra):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    kw = dict(resample=True, resample_temperature=TEMP, resample_u=U)
    kw.update(extra)
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3, use_graph=True,
                                  backend=ResampleOracleBackend(ahv, oracle), want_scores=True, **kw)
    assert not c2f.use_graph  # CPU tensors / gloo: eager
    out = [t.clone().numpy() for t in c2f(vs, vt)]
    return c2f, out


def test_resample_argument_is_checked(ahv, oracle):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, backend=ResampleOracleBackend(ahv, oracle), **kw)
    with pytest.raises(RuntimeError, match="seeds"):
        mk(resample=True, seeds=2)
    with pytest.raises(RuntimeError, match="modes"):
        mk(resample=True, modes=4)
    with pytest.raises(RuntimeError, match="fused"):
        ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, fused=True, resample=True)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="temperature"):
            mk(resample=True, resample_temperature=bad)
    for bad in (1.0, -0.5, torch.zeros(2), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="resample_u"):
            mk(resample=True, resample_u=bad)
    assert mk().resample is False and mk(resample=True).resample is True and mk(resample=True).seeds == 1


def test_resample_step_world1(ahv, oracle):
    c2f, out = _run(ahv, oracle)
    score, idx, R_pred, c_score, c_idx = out
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    one = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3,
                                  backend=ResampleOracleBackend(ahv, oracle), want_scores=True)
    ref1 = [t.clone().numpy() for t in one(vs, vt)]
    s1 = c2f.last["coarse_scores"].numpy()
    draws = c2f.last["resample"].numpy()
    assert draws.shape == (3, N_FINE) and draws.dtype == np.int64
    # the coarse stage is the single-seed step's; slot 0 is its arg-max, the other slots are the reference's draws
    assert np.array_equal(s1, one.last["coarse_scores"].numpy())
    assert np.array_equal(c_idx, ref1[4]) and np.array_equal(c_score, ref1[3]) and np.array_equal(c_idx, s1.argmax(axis=1))
    want = rr.resample(s1, N_FINE, TEMP, U)
    assert np.array_equal(draws[:, 0], c_idx) and np.array_equal(draws[:, 1:], want[:, 1:])
    assert all(len(set(d.tolist())) > 3 for d in draws)      # the draws spread: the feature does something on this input
    for b in range(3):
        rr.check_draws(want[b], s1[b], rr.beta_of(TEMP), U)
    # draw j is refined by D[j]
    Rf = c2f.last["R_fine"].numpy()
    want_Rf = np.matmul(c2f.R_coarse.numpy().astype(np.float64)[draws], c2f.D.numpy().astype(np.float64)[None])
    assert np.abs(Rf - want_Rf).max() <= 5 * 2.0 ** -24      # three products and two adds on entries <= 1
    s2 = c2f.last["fine_scores"].numpy()
    assert s2.shape == (3, N_FINE)
    assert np.array_equal(score, s2.max(axis=1)) and np.array_equal(idx, s2.argmax(axis=1))
    assert np.all((idx >= 0) & (idx < N_FINE))
    assert np.array_equal(R_pred, Rf[np.arange(3), idx])
    assert np.all(score >= c_score - 1e-6)   # D[0] = I and slot 0 is the arg-max: never below the coarse winner
    again = [t.clone().numpy() for t in c2f(vs, vt)]
    for a, b in zip(again, out):
        assert np.array_equal(a, b)


def test_resample_default_offset_and_tensor_offset(ahv, oracle):
    a, out_a = _run(ahv, oracle, resample_u=None)
    b, out_b = _run(ahv, oracle, resample_u=torch.full((3,), 0.5))
    assert np.array_equal(a.last["resample"].numpy(), b.last["resample"].numpy())
    for x, y in zip(out_a, out_b):
        assert np.array_equal(x, y)
    c, _ = _run(ahv, oracle, resample_u=torch.tensor([0.0, 0.5, 0.75]))
    want = rr.resample(c.last["coarse_scores"].numpy(), N_FINE, TEMP, np.array([0.0, 0.5, 0.75], np.float32))
    assert np.array_equal(c.last["resample"].numpy()[:, 1:], want[:, 1:])


def test_resample_off_is_the_single_seed_step(ahv, oracle):
    """The regression guard: resample=False leaves the seeds=1 step's results as they are."""
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3,
                                              backend=ResampleOracleBackend(ahv, oracle), want_scores=True, **kw)
    a, b = mk(), mk(resample=False, resample_temperature=0.5, resample_u=0.9)
    for x, y in zip(a(vs, vt), b(vs, vt)):
        assert torch.equal(x, y)
    assert torch.equal(a.last["fine_scores"], b.last["fine_scores"]) and "resample" not in b.last


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
        # TWO exchanges per step: the coarse-score gather, then the (B,) fine key
        assert calls == [("all_gather", (3, -(-N_COARSE // world))), ("all_reduce", (3,))], calls
        q.put((rank, (c2f.c_lo, c2f.c_hi, c2f.f_lo, c2f.f_hi), out, c2f.last["resample"].numpy(),
               c2f.last["coarse_scores"].numpy(), c2f.last["fine_scores"].numpy()))
    finally:
        dist.destroy_process_group()


def test_resample_step_world2_equals_single_rank(ahv, oracle):
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
    names = ["fine score", "fine index", "R_pred", "coarse score", "coarse index"]
    for rank, (c_lo, c_hi, f_lo, f_hi), out, draws, s1, s2 in got:
        for name, a, b in zip(names, out, ref):
            assert np.array_equal(a, b), (rank, name)
        assert np.array_equal(draws, single.last["resample"].numpy()), rank       # the same draw list on every rank
        assert (c_lo, c_hi) == ahv.dist.shard_range(N_COARSE, rank, world)
        assert (f_lo, f_hi) == ahv.dist.shard_range(N_FINE, rank, world)
        assert np.array_equal(s1, single.last["coarse_scores"].numpy())           # the gathered row is the whole row
        assert np.array_equal(s2, single.last["fine_scores"].numpy()[:, f_lo:f_hi])
