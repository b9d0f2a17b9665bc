"""K-best hypotheses, CPU tier: argument validation of the four top-K launches through the ctypes table (validation runs
before any HIP call), the list order on the host codec, and ``CoarseToFine(seeds=K)``'s control flow on an oracle-backed CPU
backend -- world 1, and world 2 under gloo against world 1 (same coarse list, same fine winner, same R_pred, bit for bit)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from .conftest import REPO
from .test_dist_cpu import _free_port
from .test_refine_dist_cpu import OracleBackend, _inputs

N_COARSE, N_FINE, SEEDS = 96, 40, 4


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def host_topk(ahv, keys: np.ndarray, k: int) -> np.ndarray:
    """(B, M) int64 candidate keys -> (B, k): the k largest DISTINCT keys, descending, EMPTY-padded (the merge rule)."""
    out = np.full((keys.shape[0], k), ahv.dist.KEY_EMPTY, dtype=np.int64)
    for b in range(keys.shape[0]):
        u = np.unique(keys[b])[::-1]
        u = u[u != ahv.dist.KEY_EMPTY][:k]
        out[b, :len(u)] = u
    return out


class TopkOracleBackend(OracleBackend):
    """The CPU backend protocol with the four list operations ``seeds > 1`` calls, on the host key codec."""

    def topk(self, scores, k, n_offset=0, keys=None, reset=None):
        s = scores.numpy()
        idx = np.broadcast_to(np.arange(s.shape[1], dtype=np.int64) + n_offset, s.shape)
        cand = self.ahv.dist.pack_keys_host(s, idx).reshape(s.shape)
        if keys is not None and not reset:
            cand = np.concatenate([cand, keys.numpy()], axis=1)
        new = torch.from_numpy(host_topk(self.ahv, cand, k))
        if keys is None:
            return new
        keys.copy_(new)
        return keys

    def merge_topk(self, lists, keys=None, reset=None):
        P, B, k = lists.shape
        cand = lists.numpy().transpose(1, 0, 2).reshape(B, P * k)
        if keys is not None and not reset:
            cand = np.concatenate([cand, keys.numpy()], axis=1)
        new = torch.from_numpy(host_topk(self.ahv, cand, k))
        if keys is None:
            return new
        keys.copy_(new)
        return keys

    def select_topk(self, keys, R, n_offset=0, reset_keys=False):
        s, i = self.ahv.dist.unpack_keys_host(keys.numpy())
        B, k = keys.shape
        N = R.shape[-3]
        out = torch.zeros(B, k, 3, 3)
        for b in range(B):
            for j in range(k):
                loc = int(i[b, j]) - n_offset
                if 0 <= loc < N:
                    out[b, j] = R[b, loc] if R.dim() == 4 else R[loc]
        if reset_keys:
            keys.fill_(self.ahv.dist.KEY_EMPTY)
        return torch.from_numpy(s), torch.from_numpy(i), out

    def compose_rotations_topk(self, keys, R, D, n_offset=0, out=None):
        _, i = self.ahv.dist.unpack_keys_host(keys.numpy())
        B, k = keys.shape
        loc = torch.from_numpy(i) - n_offset
        loc = torch.where((loc < 0) | (loc >= R.shape[-3]), torch.zeros_like(loc), loc)
        seeds = R[loc]                                                  # (B, k, 3, 3)
        r = torch.matmul(seeds[:, :, None], D[None, None]).reshape(B, k * D.shape[0], 3, 3).contiguous()
        if out is not None:
            out.copy_(r)
            return out
        return r


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------

def test_topk_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    ws_bytes = lib.ahv_topk_workspace_bytes
    # the workspace size is a pure function of (B, N, K): partial lists of up to 63 workgroups per sample, 1024 scores each
    assert ws_bytes(0, 50_000, 16) == 0 and ws_bytes(3, 0, 16) == 0
    assert ws_bytes(3, 50_000, 0) == 0 and ws_bytes(3, 50_000, 65) == 0
    assert ws_bytes(1, 1000, 64) == 0                       # one tile: one launch, no scratch
    assert ws_bytes(1, 50_000, 16) == 8 * 49 * 16 == ws_bytes(1, 50_000, 16)
    assert ws_bytes(32, 50_000, 64) == 8 * 49 * 32 * 64
    assert ws_bytes(2, 1_000_000, 5) == 8 * 63 * 2 * 5      # capped at 63 lists per sample

    topk = lib.ahv_topk_f32     # (scores, B, N, n_offset, K, keys, workspace, workspace_bytes, flags, stream)
    for bad in (0, 65, -1):
        assert topk(1, 1, 10, 0, bad, 1, None, 0, 0, None) == -1 and b"K" in err() and str(bad).encode() in err()
    assert topk(None, 1, 10, 0, 4, 1, None, 0, 0, None) == -1 and b"null" in err()
    assert topk(1, 1, 10, 0, 4, None, None, 0, 0, None) == -1 and b"null" in err()
    assert topk(1, -1, 10, 0, 4, 1, None, 0, 0, None) == -1 and b"negative" in err()
    assert topk(1, 1, 10, 1 << 32, 4, 1, None, 0, 0, None) == -1 and b"32 bits" in err()
    assert topk(1, 1, 10, 0, 4, 1, None, 0, 2, None) == -1 and b"flags" in err()
    assert topk(1, 1, 50_000, 0, 4, 1, None, 0, 0, None) == -1 and b"workspace" in err()
    assert topk(1, 1, 50_000, 0, 4, 1, 8, 100, 0, None) == -1 and b"workspace" in err()
    assert topk(1, 1, 50_000, 0, 4, 1, 12, 1 << 20, 0, None) == -1 and b"aligned" in err()
    assert topk(None, 0, 10, 0, 4, None, None, 0, 0, None) == 0   # B = 0: nothing to do
    assert topk(None, 2, 0, 0, 4, 1, None, 0, 0, None) == 0       # N = 0 without the reset flag: the list stays

    merge = lib.ahv_topk_merge_keys     # (lists, P, B, K, keys, flags, stream)
    for bad in (0, 65):
        assert merge(1, 2, 1, bad, 1, 0, None) == -1 and b"K" in err() and str(bad).encode() in err()
    assert merge(None, 2, 1, 4, 1, 0, None) == -1 and b"null" in err()
    assert merge(1, 2, 1, 4, None, 0, None) == -1 and b"null" in err()
    assert merge(1, -2, 1, 4, 1, 0, None) == -1 and b"negative" in err()
    assert merge(1, 2, 1, 4, 1, 4, None) == -1 and b"flags" in err()
    assert merge(None, 2, 0, 4, None, 0, None) == 0
    assert merge(None, 0, 2, 4, 1, 0, None) == 0

    sel = lib.ahv_select_topk_f32   # (keys, K, R, r_stride, n_offset, N, B, R_out, scores_out, idx_out, flags, stream)
    for bad in (0, 65):
        assert sel(1, bad, 1, 0, 0, 10, 1, 1, 1, 1, 0, None) == -1 and b"K" in err() and str(bad).encode() in err()
    assert sel(None, 4, 1, 0, 0, 10, 1, 1, 1, 1, 0, None) == -1 and b"null" in err()
    assert sel(1, 4, None, 0, 0, 10, 1, 1, 1, 1, 0, None) == -1 and b"rotation set" in err()
    assert sel(1, 4, 1, 5, 0, 10, 1, 1, 1, 1, 0, None) == -1 and b"r_batch_stride" in err()
    assert sel(1, 4, 1, 0, 0, 10, 1, 1, 1, 1, 2, None) == -1 and b"flags" in err()
    assert sel(None, 4, None, 0, 0, 10, 0, None, None, None, 0, None) == 0

    comp = lib.ahv_compose_rotations_topk_f32   # (keys, K, R, r_stride, n_offset, N, D, N2, B, out, stream)
    for bad in (0, 65):
        assert comp(1, bad, 1, 0, 0, 10, 1, 5, 1, 1, None) == -1 and b"K" in err() and str(bad).encode() in err()
    assert comp(None, 4, 1, 0, 0, 10, 1, 5, 1, 1, None) == -1 and b"null" in err()
    assert comp(1, 4, 1, 0, 0, 10, 1, 5, 1, None, None) == -1 and b"null" in err()
    assert comp(1, 4, 1, 89, 0, 10, 1, 5, 1, 1, None) == -1 and b"r_batch_stride" in err()
    assert comp(1, 4, 1, 0, 0, 0, 1, 5, 1, 1, None) == -1 and b"empty rotation set" in err()
    assert comp(1, 4, 1, 0, 0, 10, 1, 0, 1, 1, None) == 0
    assert lib.ahv_abi_version() == (2 << 16) | 3   # the entry points were added under 2.3: callers probe for the symbol


def test_topk_ops_refuse_cpu_tensors(ahv):
    keys = torch.full((2, 4), ahv.dist.KEY_EMPTY, dtype=torch.int64)
    R = torch.eye(3)[None].repeat(8, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.topk(torch.zeros(2, 8), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.merge_topk(keys[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.select_topk(keys, R)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.compose_rotations_topk(keys, R, R)
    with pytest.raises(RuntimeError, match="K = 65"):
        ahv.ops.topk(torch.zeros(2, 8), 65)


def test_list_order_is_the_stable_descending_sort(ahv):
    """The order the kernels implement, on the host codec: descending signed key order = torch.sort(descending, stable)
    truncated to K, with ties, NaNs of both signs, +-inf and +-0 -- index for index."""
    rng = np.random.default_rng(5)
    s = rng.standard_normal(5000).astype(np.float32)
    s[rng.integers(0, 5000, 300)] = s[rng.integers(0, 5000, 300)]   # ~300 ties
    s[[7, 1200, 3100]] = np.nan
    s.view(np.uint32)[4000] = 0xFFC00001                               # a NaN with the sign bit set
    s[[10, 11]] = np.inf
    s[[20, 4999]] = -np.inf
    s[[30, 31, 32]] = [0.0, -0.0, 0.0]
    keys = ahv.dist.pack_keys_host(s, np.arange(5000))
    order = np.argsort(keys)[::-1]
    assert len(np.unique(keys)) == 5000
    want = torch.sort(torch.from_numpy(s), descending=True, stable=True).indices.numpy()
    assert np.array_equal(order, want)
    got_s, got_i = ahv.dist.unpack_keys_host(host_topk(ahv, keys[None], 64))
    assert np.array_equal(got_i[0], want[:64])
    assert np.array_equal(np.isnan(got_s[0]), np.isnan(s[want[:64]]))


# ---- CoarseToFine(seeds=K) on the CPU backend --------------------------------------------------------------

def _run(ahv, oracle, seeds=SEEDS, backend=TopkOracleBackend, **extra):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    c2f = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, max_angle_deg=12.0, batch=3, use_graph=True,
                                  backend=backend(ahv, oracle), want_scores=True, **({"seeds": seeds} if seeds else {}),
                                  **extra)
    assert not c2f.use_graph  # CPU tensors / gloo: eager
    out = [t.clone().numpy() for t in c2f(vs, vt)]
    return c2f, out


def test_seeds_one_is_the_object_built_without_the_argument(ahv, oracle):
    a, out_a = _run(ahv, oracle, seeds=1)
    b, out_b = _run(ahv, oracle, seeds=None)
    c, out_c = _run(ahv, oracle, seeds=None, backend=OracleBackend)   # the four list operations are never called
    assert a.seeds == b.seeds == c.seeds == 1
    for x, y, z in zip(out_a, out_b, out_c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert "coarse_topk" not in a.last
    assert np.array_equal(a.last["fine_scores"].numpy(), c.last["fine_scores"].numpy())


def test_seeds_argument_is_checked(ahv, oracle):
    vs, vt, W1, W2, b2, R = _inputs(ahv)
    for bad in (0, 65, N_COARSE + 1):
        with pytest.raises(RuntimeError, match="seeds"):
            ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, backend=TopkOracleBackend(ahv, oracle), seeds=bad)
    with pytest.raises(RuntimeError, match="fused"):
        ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N_FINE, batch=3, fused=True, seeds=4)


def test_multi_seed_step_world1(ahv, oracle):
    c2f, (score, idx, R_pred, c_score, c_idx) = _run(ahv, oracle)
    one, ref1 = _run(ahv, oracle, seeds=1)
    s1 = c2f.last["coarse_scores"].numpy()
    top_s, top_i = (t.numpy() for t in c2f.last["coarse_topk"])
    want = torch.sort(torch.from_numpy(s1), dim=1, descending=True, stable=True).indices.numpy()[:, :SEEDS]
    assert np.array_equal(top_i, want)
    assert np.array_equal(top_s, np.take_along_axis(s1, want, axis=1))
    assert np.array_equal(c_idx, ref1[4]) and np.array_equal(c_score, ref1[3])   # first entry = the arg-max
    # the composed set: K blocks of N2, block k around seed k; block 0 is the single-seed object's refinement set
    Rf = c2f.last["R_fine"].numpy()
    assert Rf.shape == (3, SEEDS * N_FINE, 3, 3)
    want_Rf = torch.matmul(c2f.R_coarse[torch.from_numpy(top_i)][:, :, None], c2f.D[None, None]).reshape(3, -1, 3, 3)
    assert np.array_equal(Rf, want_Rf.numpy())
    s2 = c2f.last["fine_scores"].numpy()
    assert np.array_equal(s2[:, :N_FINE], one.last["fine_scores"].numpy())
    assert np.all(score >= ref1[0])             # seed 0 is the arg-max: more seeds never score below one
    assert np.array_equal(idx, np.argmax(s2, axis=1)) and np.array_equal(score, s2.max(axis=1))
    assert np.array_equal(R_pred, Rf[np.arange(3), idx])
    assert np.all((0 <= idx) & (idx < SEEDS * N_FINE))
    # the keys and the list are handed back / rebuilt: a second step gives the same answer
    vs, vt = _inputs(ahv)[:2]
    again = [t.clone().numpy() for t in c2f(vs, vt)]
    for a, b in zip(again, (score, idx, R_pred, c_score, c_idx)):
        assert np.array_equal(a, b)


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
        # still TWO exchanges per step: the (B,K) list all-gather in place of the coarse key all-reduce, then the fine key
        assert calls == [("all_gather", (3, SEEDS)), ("all_reduce", (3,))], calls
        q.put((rank, (c2f.c_lo, c2f.c_hi, c2f.f_lo, c2f.f_hi), out, [t.numpy() for t in c2f.last["coarse_topk"]],
               c2f.last["coarse_scores"].numpy(), c2f.last["fine_scores"].numpy()))
    finally:
        dist.destroy_process_group()


def test_multi_seed_step_world2_equals_single_rank(ahv, oracle):
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
    names = ["fine score", "fine index", "R_pred", "coarse score", "coarse index"]
    for rank, (c_lo, c_hi, f_lo, f_hi), out, top, s1, s2 in got:
        for name, a, b in zip(names, out, ref):
            assert np.array_equal(a, b), (rank, name)
        assert np.array_equal(top[0], ref_top[0]) and np.array_equal(top[1], ref_top[1]), rank   # the same coarse list
        assert (c_lo, c_hi) == ahv.dist.shard_range(N_COARSE, rank, world)
        assert (f_lo, f_hi) == ahv.dist.shard_range(SEEDS * N_FINE, rank, world)
        assert np.array_equal(s1, single.last["coarse_scores"].numpy()[:, c_lo:c_hi])
        assert np.array_equal(s2, single.last["fine_scores"].numpy()[:, f_lo:f_hi])
