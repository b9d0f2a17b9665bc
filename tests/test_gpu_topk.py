"""K-best hypotheses on the GPU: the top-K selection kernels (``ahv_topk_f32``, ``ahv_topk_merge_keys``, ``ahv_select_topk_f32``,
``ahv_compose_rotations_topk_f32``) through the C ABI, and the multi-seed coarse-to-fine step built on them.

The order under test is ``torch.sort(scores, dim=1, descending=True, stable=True)`` truncated to K (NaN first, lowest index
among equal scores, -0 = +0) -- computed on the CPU here; it is NOT ``torch.topk``'s order (ties unspecified there)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from .conftest import GOLDEN, REPO, load_golden

pytestmark = pytest.mark.gpu

EMPTY = -(1 << 63)


@pytest.fixture(scope="module")
def setup(ahv, g128):
    dev = torch.device("cuda:0")
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k])).to(dev)
    g = np.load(os.path.join(GOLDEN, "batched.npz"))
    vs, vt = torch.from_numpy(g["vol_src"]).to(dev), torch.from_numpy(g["vol_tgt"]).to(dev)
    return dev, vs, vt, T("W1"), T("W2"), T("b2")


def make_scores(B, N, seed, nonpositive=False):
    """Random scores with planted ties (also among the largest values), NaNs of both signs, +-inf and +-0."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, N)).astype(np.float32)
    if nonpositive:
        s = -np.abs(s)   # +-0 are then the largest finite values: they reach the list
    for b in range(B):
        if N >= 8:
            n_ties = max(2, min(300, N // 8))
            s[b, rng.integers(0, N, n_ties)] = s[b, rng.integers(0, N, n_ties)]
            top = np.sort(s[b])[-min(10, N):]
            s[b, rng.integers(0, N, 6)] = np.repeat(top[[0, len(top) // 2, -1]], 2)   # ties inside the first ranks
            p = rng.choice(N, 8, replace=False)
            s[b, p[0]] = np.inf
            s[b, p[1]] = -np.inf
            s[b, p[2]], s[b, p[3]] = 0.0, -0.0
            if b % 2 == 0:
                s[b, p[4]] = np.nan
                s[b].view(np.uint32)[p[5]] = 0xFFC00000   # NaN with the sign bit set
                s[b].view(np.uint32)[p[6]] = 0x7F800001   # a signalling NaN pattern
                s[b].view(np.uint32)[p[7]] = 0xFFFFFFFF
        elif N >= 3:
            s[b, 0], s[b, 1], s[b, 2] = -0.0, 0.0, -0.0
    return s


def expected_list(s, K, n_offset=0):
    """(idx (B,K) global int64 with -1 padding, scores (B,K) with -inf padding) of the stable descending sort."""
    B, N = s.shape
    order = torch.sort(torch.from_numpy(s), dim=1, descending=True, stable=True).indices.numpy()[:, :K]
    idx = np.full((B, K), -1, dtype=np.int64)
    sc = np.full((B, K), -np.inf, dtype=np.float32)
    m = min(N, K)
    idx[:, :m] = order[:, :m] + n_offset
    with np.errstate(invalid="ignore"):   # a signalling NaN in the sum
        sc[:, :m] = np.take_along_axis(s, order[:, :m], axis=1) + np.float32(0.0)   # -0 is reported as +0 (pack_key)
    return idx, sc


def assert_scores_bitwise(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- order semantics ---------------------------------------------------------------------------------------

CASES = [  # (B, N, K, n_offset, nonpositive)
    (1, 3, 5, 0, False), (3, 2, 64, 11, True), (3, 64, 64, 0, False), (1, 5, 5, 3, True),
    (1, 50_000, 1, 0, False), (1, 50_000, 5, 0, False), (1, 50_000, 64, 0, False), (3, 50_000, 64, 0, True),
    (1, 200_000, 64, 0, False), (3, 200_000, 5, 1, False), (32, 50_000, 5, 0, False), (32, 50_000, 64, 7, False),
    (3, 4099, 5, 13, False), (3, 2045, 64, 1, True), (32, 2047, 1, 5, False), (1, 2048, 64, 0, False),
    (3, 131_073, 64, 999, True), (3, 1021, 64, 1, True), (32, 1023, 1, 5, False), (1, 1024, 64, 0, False),
    (3, 1025, 16, 2, False), (1, 64_513, 64, 0, False),
]


@pytest.mark.parametrize("B,N,K,n_offset,nonpositive", CASES)
def test_order_is_the_stable_descending_sort(ahv, setup, B, N, K, n_offset, nonpositive):
    dev = setup[0]
    s = make_scores(B, N, seed=B * 1000 + N + K, nonpositive=nonpositive)
    want_idx, want_sc = expected_list(s, K, n_offset)
    sd = torch.from_numpy(s).to(dev)
    keys = ahv.ops.topk(sd, K, n_offset=n_offset)
    assert keys.shape == (B, K) and keys.dtype == torch.int64
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(N, 3)).to(dev)
    sc, idx, Rk = ahv.ops.select_topk(keys, R, n_offset=n_offset)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(idx, want_idx)
    assert_scores_bitwise(sc, want_sc)
    # keys are strictly descending up to the padding; the padding is AHV_KEY_EMPTY and decodes to (-inf, -1, zero row)
    k = keys.cpu().numpy()
    m = min(N, K)
    assert np.all(k[:, 1:m] < k[:, :m - 1]) and np.all(k[:, m:] == EMPTY)
    want_R = torch.zeros(B, K, 3, 3, device=dev)
    want_R[:, :m] = R[torch.from_numpy(want_idx[:, :m] - n_offset).to(dev)]
    assert torch.equal(Rk, want_R)
    # the host codec agrees with the device on every key
    hk = ahv.dist.pack_keys_host(want_sc[:, :m], want_idx[:, :m]).reshape(B, m)
    assert np.array_equal(k[:, :m], hk)
    # first entry = the arg-max key
    if N > 0:
        assert torch.equal(keys[:, 0], ahv.ops.argmax(sd, n_offset=n_offset, return_key=True))


def test_k_out_of_range_is_refused(ahv, setup):
    s = torch.zeros(2, 100, device=setup[0])
    for bad in (0, 65):
        with pytest.raises(RuntimeError, match="K = %d" % bad):
            ahv.ops.topk(s, bad)
    lib = ahv._lib.load()
    keys = torch.empty(2, 64, dtype=torch.int64, device=setup[0])
    assert lib.ahv_topk_f32(s.data_ptr(), 2, 100, 0, 65, keys.data_ptr(), None, 0, 0, None) == -1
    assert b"K" in lib.ahv_last_error()


# ---- composition: whole = chunked merge-into = merge of per-shard lists -------------------------------------------------

@pytest.mark.parametrize("B,N,K", [(3, 50_000, 64), (1, 20_011, 5), (32, 9_001, 16)])
def test_chunks_and_shards_compose(ahv, setup, B, N, K):
    dev = setup[0]
    s = make_scores(B, N, seed=N + K)
    sd = torch.from_numpy(s).to(dev)
    whole = ahv.ops.topk(sd, K)
    # 7 uneven chunks merged into one list, in a scrambled order (the rule is order-free)
    cuts = np.unique(np.concatenate([[0, N], np.random.default_rng(1).integers(1, N, 6)]))
    assert len(cuts) == 8
    keys = torch.full((B, K), EMPTY, dtype=torch.int64, device=dev)
    for j in [3, 0, 6, 2, 5, 1, 4]:
        lo, hi = int(cuts[j]), int(cuts[j + 1])
        out = ahv.ops.topk(sd[:, lo:hi], K, n_offset=lo, keys=keys)   # a strided view: ops makes it contiguous
        assert out is keys
    assert torch.equal(keys, whole)
    # merging the same chunk again changes nothing (a key met twice is kept once); reset starts over
    ahv.ops.topk(sd[:, :int(cuts[1])], K, n_offset=0, keys=keys)
    assert torch.equal(keys, whole)
    ahv.ops.topk(sd[:, :int(cuts[1])], K, n_offset=0, keys=keys, reset=True)
    assert torch.equal(keys, ahv.ops.topk(sd[:, :int(cuts[1])].contiguous(), K))
    # 8 shards, one of them listed twice, through merge_topk
    lists = []
    for r in range(8):
        lo, hi = ahv.dist.shard_range(N, r, 8)
        lists.append(ahv.ops.topk(sd[:, lo:hi], K, n_offset=lo))
    lists.append(lists[2])
    merged = ahv.ops.merge_topk(torch.stack(lists))
    assert torch.equal(merged, whole)
    # merge-into: half the shards first, the rest into the same list
    half = ahv.ops.merge_topk(torch.stack(lists[:4]))
    ahv.ops.merge_topk(torch.stack(lists[3:]), keys=half)
    assert torch.equal(half, whole)
    assert torch.equal(whole[:, 0], ahv.ops.argmax(sd, return_key=True))


# ---- reference fixtures ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["score_n128", "score_n4096"])
def test_verify_pair_topk_against_the_reference_scores(ahv, setup, g128, name):
    """K = 64 on the G1 volumes and weights.  A rank is left out of the exact-order comparison only when the reference gap to
    a neighbour is below 2e-6 (ten times the ~2e-7 absolute agreement of scores of this size); on these fixtures that is no
    rank at all (smallest gap among the first 65 reference scores: 9.5e-6 / 6.1e-6), and the test asserts so."""
    dev, _, _, W1, W2, b2 = setup
    g = load_golden(name)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vs, vt, R = T(g128["vol_src"]), T(g128["vol_tgt"]), T(g["R"])
    ref = np.asarray(g["scores"], dtype=np.float32)
    K = 64
    scores, best_key, keys = ahv.ops.verify_pair_topk(vs, vt, R, W1, W2, b2, K)
    assert torch.equal(keys[:, 0], best_key)
    sc, idx, Rk = ahv.ops.select_topk(keys, R)
    order = torch.sort(torch.from_numpy(ref), dim=1, descending=True, stable=True).indices.numpy()
    top = np.take_along_axis(ref, order[:, :K + 1], axis=1).astype(np.float64)
    gaps = top[:, :-1] - top[:, 1:]                      # gap of rank r to rank r + 1, r < K
    print("%s: smallest gap among the first %d reference scores %.3e" % (name, K + 1, gaps.min()))
    close = gaps < 2e-6
    left_out = np.zeros((1, K), dtype=bool)
    left_out |= close[:, :K]
    left_out[:, 1:] |= close[:, :K - 1]
    assert int(left_out.sum()) == 0
    assert np.array_equal(idx.cpu().numpy()[~left_out], order[:, :K][~left_out])
    want = np.take_along_axis(ref, order[:, :K], axis=1)
    got = sc.cpu().numpy()
    rel = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-2)))
    print("%s: decoded scores max rel err %.3e" % (name, rel))
    assert rel < 1e-4
    assert torch.equal(sc, torch.gather(scores, 1, idx)) and torch.equal(Rk, R[idx])
    # the feature-level twin gives the same list
    ft = ahv.ops.forward_3d2d(vt, W1, W2, b2)
    s2, key2, keys2 = ahv.ops.score_hypotheses_topk(vs, ft, R, W1, W2, b2, K)
    assert torch.equal(keys2[:, 0], key2)
    assert np.array_equal(ahv.ops.select_topk(keys2, R)[1].cpu().numpy()[~left_out], order[:, :K][~left_out])


# ---- select / compose ------------------------------------------------------------------------------------------------

def host_compose(Rs, D):
    """The kernel's expression as the compiler contracts it (mul, fma, fma -- read off the gfx950 code):
    o[a][c] = fma(r[a][2], d[2][c], fma(r[a][1], d[1][c], fl(r[a][0] * d[0][c]))).  An fp32 fma is emulated as the fp32
    rounding of the float64 value of a*b + c (the product is exact in float64; the sum is rounded twice), so the comparison
    allows 1 ulp at the magnitude of a rotation's entries (|x| <= 1: 2^-23) instead of asking for bit equality."""
    r = Rs[:, :, None].astype(np.float32)          # (B, K, 1, 3, 3)
    d = D[None, None].astype(np.float32)           # (1, 1, N2, 3, 3)
    f64 = lambda x: x.astype(np.float64)
    out = np.empty(np.broadcast_shapes(r.shape, d.shape), dtype=np.float32)
    for a in range(3):
        for c in range(3):
            t = (r[..., a, 0] * d[..., 0, c]).astype(np.float32)
            t = (f64(r[..., a, 1]) * f64(d[..., 1, c]) + f64(t)).astype(np.float32)
            out[..., a, c] = (f64(r[..., a, 2]) * f64(d[..., 2, c]) + f64(t)).astype(np.float32)
    return out.reshape(Rs.shape[0], -1, 3, 3)


@pytest.mark.parametrize("per_sample", [False, True])
def test_select_and_compose(ahv, setup, per_sample):
    dev = setup[0]
    B, N, N2, K = 3, 5000, 37, 8
    Rn = ahv.rotations.haar_rotations_np(B * N, 9).reshape(B, N, 3, 3)
    R = torch.from_numpy(Rn if per_sample else Rn[0]).to(dev)
    D = ahv.rotations.refine_rotations(torch.eye(3), N2, 8.0, generator=torch.Generator().manual_seed(1)).to(dev)
    s = torch.from_numpy(make_scores(B, N, seed=77)).to(dev)
    keys = ahv.ops.topk(s, K)
    sc, idx, Rk = ahv.ops.select_topk(keys, R)
    rows = torch.stack([R[b][idx[b]] for b in range(B)]) if per_sample else R[idx]
    assert torch.equal(Rk, rows)
    # sharded over 4 slices: every slice decodes the same scores / indices, the rows sum to the unsharded ones
    total = torch.zeros_like(Rk)
    for r in range(4):
        lo, hi = ahv.dist.shard_range(N, r, 4)
        sc_r, idx_r, R_r = ahv.ops.select_topk(keys, R[..., lo:hi, :, :], n_offset=lo)
        assert torch.equal(idx_r, idx) and torch.equal(sc_r.view(torch.int32), sc.view(torch.int32))
        owned = (idx >= lo) & (idx < hi)
        assert torch.equal(R_r[owned], Rk[owned]) and torch.count_nonzero(R_r[~owned]) == 0
        total += R_r
    assert torch.equal(total, Rk)
    # reset flag: the list comes back empty, the outputs are those of the plain call
    k2 = keys.clone()
    out = ahv.ops.select_topk(k2, R, reset_keys=True)
    assert torch.equal(out[1], idx) and torch.equal(out[2], Rk) and bool((k2 == EMPTY).all())
    # compose: K = 1 is compose_rotations bit for bit
    one = ahv.ops.compose_rotations_topk(keys[:, :1].contiguous(), R, D)
    assert torch.equal(one, ahv.ops.compose_rotations(keys[:, 0].contiguous(), R, D))
    # K = 8: the kernel's expression recomputed on the host, <= 1 ulp at magnitude 1 (2^-23), see host_compose
    fine = ahv.ops.compose_rotations_topk(keys, R, D)
    assert fine.shape == (B, K * N2, 3, 3)
    want = host_compose(rows.cpu().numpy(), D.cpu().numpy())
    err = float(np.max(np.abs(fine.cpu().numpy() - want)))
    print("compose K=8: max abs diff to the host expression %.3e" % err)
    assert err <= 2.0 ** -23
    assert torch.equal(fine[:, :N2], one)   # block 0 = the single-seed set
    # an empty slot composes row 0 and stays in bounds
    k3 = keys.clone()
    k3[:, -1] = EMPTY
    f3 = ahv.ops.compose_rotations_topk(k3, R, D)
    r0 = (R[:, 0] if per_sample else R[0].expand(B, 3, 3)).contiguous()
    want0 = host_compose(r0[:, None].cpu().numpy(), D.cpu().numpy())
    assert float(np.max(np.abs(f3[:, (K - 1) * N2:].cpu().numpy() - want0))) <= 2.0 ** -23


@pytest.mark.parametrize("per_sample", [False, True])
def test_single_best_decode_against_the_host_codec(ahv, setup, per_sample):
    """``select_rotation`` / ``compose_rotations`` (the list kernels at K = 1) against ``dist.unpack_keys_host`` and a torch
    gather of the rows -- not against the list calls, which run the same kernels.  B = 1, 64, 65, 257 keys cross the
    workgroup boundary (256 slots); this rank holds hypotheses 10 .. 46 of 47 (N = 37, n_offset = 10)."""
    dev = setup[0]
    NF, lo = 47, 10
    N = NF - lo
    for B in (1, 64, 65, 257):
        rng = np.random.default_rng(B)
        sc = rng.standard_normal(B).astype(np.float32)
        gi = rng.integers(lo, NF, B)
        Rn = ahv.rotations.haar_rotations_np(B * NF, 5).reshape(B, NF, 3, 3)
        R = torch.from_numpy(Rn if per_sample else Rn[0]).to(dev)[..., lo:, :, :]
        for special in ("empty", "foreign", "nan"):
            s, g = sc.copy(), gi.copy()
            at = B // 2
            if special == "foreign":
                g[at] = lo - 6          # below the slice; with B >= 64 one above it as well (a global index past n_offset + N)
                g[B - 1] = NF + 3 if B > 1 else g[B - 1]
            if special == "nan":
                s[at] = np.nan
                s[0] = -0.0 if B > 1 else s[0]
            keys = ahv.dist.pack_keys_host(s, g).reshape(B).copy()
            if special == "empty":
                keys[at] = EMPTY
            want_s, want_i = ahv.dist.unpack_keys_host(keys)
            if special == "empty":
                assert want_s[at] == -np.inf and want_i[at] == -1
            mine = torch.from_numpy((keys != EMPTY) & (want_i >= lo) & (want_i < NF)).to(dev)
            loc = torch.from_numpy(np.clip(want_i - lo, 0, N - 1)).to(dev)
            rows = R[torch.arange(B, device=dev), loc] if per_sample else R[loc]
            want_R = torch.where(mine[:, None, None], rows, torch.zeros_like(rows))
            assert int((~mine).sum()) == {"empty": 1, "foreign": 2 if B > 1 else 1, "nan": 0}[special]
            for reset in (False, True):
                k = torch.from_numpy(keys.copy()).to(dev)
                got_s, got_i, got_R = ahv.ops.select_rotation(k, R, n_offset=lo, reset_key=reset)
                assert got_s.shape == (B,) and got_i.shape == (B,) and got_R.shape == (B, 3, 3)
                assert np.array_equal(got_i.cpu().numpy(), want_i)
                assert np.array_equal(got_s.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
                assert torch.equal(got_R, want_R)
                assert np.array_equal(k.cpu().numpy(), np.full(B, EMPTY) if reset else keys)
    # compose_rotations: 5 x 67 matrices span two workgroups; an EMPTY key and a foreign one compose row 0 (stay in bounds)
    B, N2 = 5, 67
    D = ahv.rotations.refine_rotations(torch.eye(3), N2, 8.0, generator=torch.Generator().manual_seed(1)).to(dev)
    Rn = ahv.rotations.haar_rotations_np(B * NF, 6).reshape(B, NF, 3, 3)
    R = torch.from_numpy(Rn if per_sample else Rn[0]).to(dev)[..., lo:, :, :]
    g = np.array([lo, NF - 1, 23, 3, 30])
    keys = ahv.dist.pack_keys_host(np.arange(B, dtype=np.float32), g).reshape(B).copy()
    keys[4] = EMPTY
    loc = torch.tensor([0, N - 1, 23 - lo, 0, 0], device=dev)
    rows = R[torch.arange(B, device=dev), loc] if per_sample else R[loc]
    fine = ahv.ops.compose_rotations(torch.from_numpy(keys).to(dev), R, D, n_offset=lo)
    assert fine.shape == (B, N2, 3, 3)
    want = host_compose(rows[:, None].cpu().numpy(), D.cpu().numpy())
    err = float(np.max(np.abs(fine.cpu().numpy() - want)))
    print("compose_rotations: max abs diff to the host expression %.3e" % err)
    assert err <= 2.0 ** -23


# ---- the multi-seed coarse-to-fine step ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
def test_multi_seed_step_configs4_size(ahv, oracle, setup, B):
    """CoarseToFine(seeds=8, want_scores=True), 10 000 + 1 000, on the inputs of
    test_gpu_refine.py::test_configs4_full_size_graph_vs_oracle, both input orders; eager, captured, run_many."""
    dev, vs3, vt3, W1, W2, b2 = setup
    vs, vt = vs3[:B].contiguous(), vt3[:B].contiguous()
    K, N2 = 8, 1000
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(10_000, 40)).to(dev)
    mk = lambda **kw: ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=N2, max_angle_deg=10.0, batch=B, want_scores=True, **kw)
    eager, graph, many, single = mk(seeds=K, use_graph=False), mk(seeds=K, use_graph=True), mk(seeds=K, use_graph=True), \
        mk(use_graph=False)
    assert not eager.use_graph and graph.use_graph and single.seeds == 1
    W = [t.cpu().numpy() for t in (W1, W2, b2)]
    Rn, Dn = R.cpu().numpy(), eager.D.cpu().numpy()
    rel = lambda got, ref: float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-2)))
    results = []
    for rep in range(2):
        a, b = (vs, vt) if rep == 0 else (vt, vs)
        out = [t.clone() for t in eager(a, b)]
        score, idx, R_pred, c_score, c_idx = [t.cpu().numpy() for t in out]
        top_s, top_i = (t.clone().cpu().numpy() for t in eager.last["coarse_topk"])
        s1, s2 = eager.last["coarse_scores"].cpu().numpy(), eager.last["fine_scores"].clone()
        R_fine = eager.last["R_fine"].cpu().numpy()
        an, bn = a.cpu().numpy(), b.cpu().numpy()
        # (i) the coarse list = the stable descending order of the oracle's coarse scores, exactly; no rank left out
        ref1, best1, idx1 = oracle.score_hypotheses(an, bn, Rn, *W)
        order = torch.sort(torch.from_numpy(ref1), dim=1, descending=True, stable=True).indices.numpy()
        top9 = np.take_along_axis(ref1, order[:, :K + 1], axis=1).astype(np.float64)
        print("B=%d rep=%d: smallest gap among the first nine oracle scores %.3e" % (B, rep, (top9[:, :-1] - top9[:, 1:]).min()))
        assert np.array_equal(top_i, order[:, :K])
        assert rel(s1, ref1) < 1e-4 and rel(top_s, np.take_along_axis(ref1, order[:, :K], axis=1)) < 1e-4
        assert np.array_equal(c_idx, idx1) and np.array_equal(c_idx, top_i[:, 0]) and np.array_equal(c_score, top_s[:, 0])
        assert np.array_equal(top_s, np.take_along_axis(s1, top_i, axis=1))
        # (ii) the composed set, the fine scores against the oracle on it, the fine index exactly
        want_fine = np.matmul(Rn[top_i][:, :, None], Dn[None, None]).reshape(B, K * N2, 3, 3)
        assert R_fine.shape == (B, K * N2, 3, 3) and np.max(np.abs(R_fine - want_fine)) < 1e-6
        ref2, best2, idx2 = oracle.score_hypotheses(an, bn, R_fine, *W)
        assert rel(s2.cpu().numpy(), ref2) < 1e-4 and rel(score, best2) < 1e-4
        assert np.array_equal(idx, idx2), (idx, idx2, np.sort(ref2, axis=1)[:, -2:])
        assert np.array_equal(R_pred, R_fine[np.arange(B), idx2])
        # (iii) seed 0 is the arg-max: its N2 fine scores are the single-seed object's, bit for bit
        one = [t.clone() for t in single(a, b)]
        assert torch.equal(s2[:, :N2], single.last["fine_scores"])
        assert bool((out[0] >= one[0]).all()) and torch.equal(out[3], one[3]) and torch.equal(out[4], one[4])
        # (iv) replay = eager
        got = [t.clone() for t in graph(a, b)]
        for x, y in zip(got, out):
            assert torch.equal(x, y)
        assert torch.equal(graph.last["fine_scores"], s2)
        assert all(torch.equal(x, y) for x, y in zip(graph.last["coarse_topk"], eager.last["coarse_topk"]))
        results.append(out)
    # run_many = single steps
    steps = 4
    vsm = torch.stack([vs, vt, vs, vt])
    vtm = torch.stack([vt, vs, vt, vs])
    for rnd in range(2):   # the second round replays the captured graph
        outs = many.run_many(vsm, vtm, steps=steps)
        for k in range(steps):
            for x, y in zip(outs[k], results[k % 2]):
                assert torch.equal(x, y), (rnd, k)


def test_fused_with_seeds_is_refused(ahv, setup):
    dev, _, _, W1, W2, b2 = setup
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(100, 40)).to(dev)
    with pytest.raises(RuntimeError, match="fused"):
        ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=10, fused=True, seeds=2)


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
R = torch.from_numpy(ahv.rotations.haar_rotations_np(10_000, 40)).to(dev)
calls = []
real_reduce, real_gather = dist.all_reduce, dist.all_gather_into_tensor
dist.all_reduce = lambda t, *a, **k: (calls.append("all_reduce"), real_reduce(t, *a, **k))[1]
dist.all_gather_into_tensor = lambda o, t, *a, **k: (calls.append("all_gather"), real_gather(o, t, *a, **k))[1]
forced = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=1000, batch=3, seeds=8, force_collectives=True, want_scores=True)
forced_eager = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=1000, batch=3, seeds=8, force_collectives=True, use_graph=False)
plain = ahv.refine.CoarseToFine(W1, W2, b2, R, n_fine=1000, batch=3, seeds=8, use_graph=False, want_scores=True)
assert forced.collectives and forced.use_graph and forced_eager.collectives and not plain.collectives
for rep in range(3):
    a, b = (vs, vt) if rep != 1 else (vt, vs)
    ref = [t.clone() for t in plain(a, b)]
    n0 = len(calls)
    for x, y in zip([t.clone() for t in forced_eager(a, b)], ref):
        assert torch.equal(x, y), (rep, x, y)
    assert calls[n0:] == ["all_gather", "all_reduce"], calls[n0:]   # two collectives per step
    for x, y in zip([t.clone() for t in forced(a, b)], ref):
        assert torch.equal(x, y), (rep, x, y)
    assert all(torch.equal(x, y) for x, y in zip(forced.last["coarse_topk"], plain.last["coarse_topk"]))
    assert torch.equal(forced.last["fine_scores"], plain.last["fine_scores"])
torch.cuda.synchronize()
print("OK graph=%s" % forced.use_graph)
dist.destroy_process_group()
'''


def test_multi_seed_step_with_rccl_collectives_captured(tmp_path):
    """A 1-rank RCCL group with the collectives forced, in a process of its own: the list all-gather + merge and the key
    all-reduce are captured into the step's hipGraph; results equal the plain step's bit for bit."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "topk_worker.py"
    script.write_text(RANK_WORKER)
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AHV_REPO=REPO,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout
    assert "OK graph=True" in p.stdout, p.stdout


# ---- Feature_Aligner.verify_hypotheses(topk=K) -----------------------------------------------------------------

def test_verify_hypotheses_topk_under_the_reference_scripts_conditions(ahv, setup, g128):
    """Eval mode, grad on (the reference's evaluation scripts never enter no_grad): the method patch.install() adds to a
    reference-shaped class, and the mirror module's own."""
    import types
    dev, vs3, vt3, W1, W2, b2 = setup

    class RefShaped(torch.nn.Module):   # what verify_hypotheses reads of the reference's Feature_Aligner: the 2D head
        def __init__(self):
            super().__init__()
            self.feature_embedding_2d = torch.nn.Sequential(torch.nn.Conv2d(384, 32, 1, bias=False), torch.nn.ReLU(),
                                                            torch.nn.Conv2d(32, 32, 1))

        def forward_3d2d(self, x):
            raise AssertionError("not called")

    um, mm = types.ModuleType("utils"), types.ModuleType("modules.modules")
    um.rotate_volume = lambda *a, **k: None
    mm.Feature_Aligner = RefShaped
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(5000, 2)).to(dev)
    assert torch.is_grad_enabled()
    ahv.patch.install(um, mm)
    try:
        m = RefShaped().to(dev)
        with torch.no_grad():
            m.feature_embedding_2d[0].weight.copy_(W1.reshape(32, 384, 1, 1))
            m.feature_embedding_2d[2].weight.copy_(W2.reshape(32, 32, 1, 1))
            m.feature_embedding_2d[2].bias.copy_(b2)
        m.eval()
        assert m.feature_embedding_2d[0].weight.requires_grad
        scores, key, klist = m.verify_hypotheses(vs3, vt3, R, want_scores=True, topk=16)
        plain = m.verify_hypotheses(vs3, vt3, R, want_scores=True)
        none_scores = m.verify_hypotheses(vs3, vt3, R, topk=16)[0]
        m.train()
        with pytest.raises(RuntimeError, match="inference step"):
            m.verify_hypotheses(vs3, vt3, R, topk=16)
    finally:
        ahv.patch.uninstall()
    assert len(plain) == 2 and none_scores is None       # the default return value is unchanged
    assert torch.equal(plain[0], scores) and torch.equal(plain[1], key)
    assert klist.shape == (3, 16) and torch.equal(klist[:, 0], key)
    sc, idx, Rk = ahv.ops.select_topk(klist, R)
    order = torch.sort(scores.cpu(), dim=1, descending=True, stable=True).indices[:, :16]
    assert torch.equal(idx.cpu(), order)
    assert torch.equal(sc, torch.gather(scores, 1, idx)) and torch.equal(Rk, R[idx])
    b_sim, b_idx, b_R = ahv.ops.select_rotation(key, R)
    assert torch.equal(b_idx, idx[:, 0]) and torch.equal(b_sim, sc[:, 0]) and torch.equal(b_R, Rk[:, 0])
