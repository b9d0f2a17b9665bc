"""Inputs, and the one call sequence, of the recorded bytes of the pose-selection kernels (tests/golden/select_kernels_recorded.npz):
tools/gen_golden_select.py records what ``recompute`` yields and tests/test_gpu_select_bytes.py compares against it, so the
fixture holds outputs only.  The inputs are seeded numpy (``RandomState``) and ``rotations.haar_rotations_np``.  All of these
kernels are documented to give the same bytes on every run (integer atomicMax on keys, no float atomics, fixed summation orders).

B = 2 or 3 throughout (the sample stride shows) and N % 4 != 0 wherever a row can start mid-vector.  Families (the prefix of a
recorded name), each the smallest shapes at which a kernel of csrc/ahv_select.hip, ahv_views.hip or ahv_posterior.hip can go wrong:
  "key_"    argmax, topk, merge_topk, select_topk, compose_rotations_topk at N = 1, 1 021 (the second row misaligned, one tile),
            1 027 (two parts: the two-launch path) and 63 * 1024 + 5 (past the 63 partial lists), each at K = 1, 5, 64; equal
            scores, a NaN, a -0 beside a +0, a -inf and n_offset = 1 000 planted; a list carried into the next chunk's call, a
            carried merge, 70 lists in one merge (two passes)
  "modes_"  topk_modes at N = 5, at N = 1 027 with per-sample R, on a set that runs out before K; modulo C4 and modulo an axis
  "fold_"   sym_fold with and without an axis, with and without velocities, keep > 0, no angle limit, without the info outputs, and in place (out = R)
  "views_"  view_rotations; fuse_view_scores with the limit on and off, weights given (one view absent) and None, V = 1, 3, 16,
            N = 5 (every combination) and 1 027; nearest_views at K = 1 and K = V with equal traces and a NaN, two workgroups;
            gather_views plain (an index outside 0..V-1, two chunks per row) and broadcast; view_rotations_compact with the
            capacity taken from a count-only call (exactly reached), too small (overflow) and = N; fuse_view_scores_compact
  "post_"   pose_posterior with K = 0 and K = 3 anchors (one slot empty) at N = 5, 1 027, 63 * 1024 + 5, every output of the
            finish and the state; a sample whose scores are all -inf; merge_posterior fresh and carried
  "res_"    resample at N = 5, 1 027, 4 099 (the largest N of tests/test_gpu_resample.py) with M = 1, 64 (u given), 1 000; a
            stretch of -inf and one of scores whose weights underflow; compose_rotations_indexed
  "asc_"    so3_ascent_candidates and so3_ascent_select at 3 and 257 seeds (a second workgroup); a zero and a NaN gradient
What is stored per output: all of it as int32 words where it is at most 48 KB, else a sha256 of its bytes plus its first and
last 256 words -- the fixture stays under 256 KB.
"""
import hashlib
import importlib

import numpy as np

rot = importlib.import_module("3dahv_amd.rotations")

FAMILIES = ("key_", "modes_", "fold_", "views_", "post_", "res_", "asc_")
WHOLE_MAX_BYTES = 48 * 1024
END_WORDS = 256
N_PARTS = 63 * 1024 + 5                                    # past the 63 partial lists / states of a sample
KEY_NS, KEY_KS, KEY_OFFSET = (1, 1021, 1027, N_PARTS), (1, 5, 64), 1000
RES_NS, RES_MS = (5, 1027, 4099), (1, 64, 1000)
TEMPERATURE = 0.1


def unpack(recorded):
    """The fixture as {name: flat int32 words}."""
    ends = np.cumsum(recorded["sizes"])
    words = recorded["words"]
    return {str(n): words[e - k:e] for n, k, e in zip(recorded["names"], recorded["sizes"], ends)}


def _entries(name, out):
    """(name, int32 words) of what is stored for the output ``out`` of case ``name``."""
    import torch
    w = out.detach().contiguous().cpu().reshape(-1).view(torch.int32).numpy()
    if w.nbytes <= WHOLE_MAX_BYTES:
        yield name, w
        return
    yield name + "_sha256", np.frombuffer(hashlib.sha256(w.tobytes()).digest(), np.int32)
    yield name + "_first", w[:END_WORDS]
    yield name + "_last", w[-END_WORDS:]


def small_rotations(n, max_deg, rs):
    """(n,3,3) float64 rotations by up to ``max_deg`` about random axes (Rodrigues)."""
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.radians(rs.uniform(0.0, max_deg, n))
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -u[:, 2], u[:, 1], u[:, 2], -u[:, 0], -u[:, 1], u[:, 0]
    return np.eye(3) + np.sin(a)[:, None, None] * K + (1.0 - np.cos(a))[:, None, None] * (K @ K)


def clustered(centres, n, max_deg, rs, between=None):
    """(n,3,3) float32: hypothesis i = centres[i % C] (@ between[i], a symmetry element) @ a rotation by up to ``max_deg``."""
    c = np.asarray(centres, np.float64)[np.arange(n) % len(centres)]
    if between is not None:
        c = c @ np.asarray(between, np.float64)
    return (c @ small_rotations(n, max_deg, rs)).astype(np.float32)


def z_turns(n, rs):
    a = rs.uniform(0.0, 2.0 * np.pi, n)
    z = np.zeros((n, 3, 3))
    z[:, 0, 0], z[:, 0, 1], z[:, 1, 0], z[:, 1, 1], z[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
    return z


def key_scores(N, seed):
    """(2,N): row 0 holds three equal top scores and a NaN, row 1 is negative but for a -0 and two +0, and holds a -inf."""
    rs = np.random.RandomState(seed)
    s = rs.uniform(-1.0, 1.0, (2, N)).astype(np.float32)
    s[1] = -np.abs(s[1]) - np.float32(0.1)
    if N == 1:
        s[1, 0] = -0.0
        return s
    s[0, [3, 300, N - 1]] = 2.0
    s[0, N // 2] = np.nan
    s[1, 5], s[1, 9], s[1, N - 2], s[1, 2] = -0.0, 0.0, 0.0, -np.inf
    return s


def _per_sample(N, seed):
    return rot.haar_rotations_np(2 * N, seed).reshape(2, N, 3, 3)


def _key_family(ops, dev, t):
    import torch
    D = t(rot.haar_rotations_np(2, 590)).to(dev)
    for i, N in enumerate(KEY_NS):
        s, s2 = t(key_scores(N, 500 + i)).to(dev), t(key_scores(N, 520 + i)).to(dev)
        R = t(_per_sample(N, 540 + i) if N in (1021, N_PARTS) else rot.haar_rotations_np(N, 540 + i)).to(dev)
        yield from _entries("key_N%d_argmax" % N, ops.argmax(s, n_offset=KEY_OFFSET, return_key=True))
        for K in KEY_KS:
            tag = "key_N%d_K%d_" % (N, K)
            keys = ops.topk(s, K, n_offset=KEY_OFFSET)
            yield from _entries(tag + "topk", keys)
            carried = ops.topk(s2, K, n_offset=KEY_OFFSET + N, keys=keys.clone())       # the next chunk of the same rows
            yield from _entries(tag + "topk_carried", carried)
            lists = torch.stack([keys, carried, ops.topk(s2, K, n_offset=KEY_OFFSET + N)])
            yield from _entries(tag + "merge", ops.merge_topk(lists))
            yield from _entries(tag + "merge_carried", ops.merge_topk(lists[1:].contiguous(), keys=keys.clone()))
            if N == 1027 or (N == 1 and K < 64):
                yield from _entries(tag + "compose", ops.compose_rotations_topk(carried, R, D, n_offset=KEY_OFFSET))
            # the slots of the second chunk belong to "another shard": zero rows
            held = carried.clone()
            score, idx, Rsel = ops.select_topk(held, R, n_offset=KEY_OFFSET, reset_keys=(K == 5))
            for what, out in (("scores", score), ("idx", idx), ("R", Rsel), ("keys_after", held)):
                yield from _entries(tag + "select_" + what, out)
    rs = np.random.RandomState(595)
    chunks = t(rs.uniform(-1.0, 1.0, (70, 2, 40)).astype(np.float32)).to(dev)
    lists = torch.stack([ops.topk(chunks[p], 5, n_offset=40 * p) for p in range(70)])
    yield from _entries("key_merge_P70_K5", ops.merge_topk(lists))


def _modes_family(ops, dev, t):
    rs = np.random.RandomState(600)
    centres = rot.haar_rotations_np(4, 601)
    sc = lambda B, N: t(rs.uniform(-1.0, 1.0, (B, N)).astype(np.float32)).to(dev)
    R5 = t(clustered(centres[:2], 5, 8.0, rs)).to(dev)
    yield from _entries("modes_N5_K3", ops.topk_modes(sc(2, 5), R5, 3, 30.0))
    one = t(clustered(centres[:1], 5, 5.0, rs)).to(dev)                    # every hypothesis within 30 degrees of the first winner
    yield from _entries("modes_N5_K4_runs_out", ops.topk_modes(sc(3, 5), one, 4, 30.0, n_offset=77))
    Rp = t(clustered(centres, 2 * 1027, 12.0, rs).reshape(2, 1027, 3, 3)).to(dev)
    s = sc(2, 1027)
    yield from _entries("modes_N1027_K5_per_sample", ops.topk_modes(s, Rp, 5, 20.0, n_offset=KEY_OFFSET))
    c4 = rot.Symmetry.cyclic(4, "Z")
    g = c4.S.numpy()[rs.randint(0, 4, 2 * 1027)]
    Rc4 = t(clustered(centres, 2 * 1027, 12.0, rs, between=g).reshape(2, 1027, 3, 3)).to(dev)
    yield from _entries("modes_N1027_K5_c4", ops.topk_modes(s, Rc4, 5, 20.0, symmetry=c4.to(dev)))
    ax = rot.Symmetry.axial("Z", flip=True)
    Rax = t(clustered(centres, 1027, 12.0, rs, between=z_turns(1027, rs))).to(dev)
    yield from _entries("modes_N1027_K3_axis", ops.topk_modes(s, Rax, 3, 20.0, symmetry=ax.to(dev)))
    yield from _entries("modes_N5_K3_axis", ops.topk_modes(sc(2, 5), R5, 3, 30.0, symmetry=rot.Symmetry.axial("Z").to(dev)))


def _fold_outputs(name, f):
    for what in ("R", "which", "elem", "trace", "V"):
        if getattr(f, what) is not None:
            yield from _entries(name + "_" + what, getattr(f, what))


def _fold_family(ops, dev, t):
    rs = np.random.RandomState(610)
    centres = rot.haar_rotations_np(3, 611)
    anchors = np.stack([centres, centres[::-1]]).astype(np.float32)           # (2,3,3,3)
    anchors[:, 1] = 0.0                                                       # an empty slot
    anchors = t(anchors).to(dev)
    c4, ax = rot.Symmetry.cyclic(4, "Z"), rot.Symmetry.axial("Z", flip=True)
    vel = lambda N: t(rs.normal(size=(2, N, 3)).astype(np.float32)).to(dev)

    def hyp(N, per, group):
        n = 2 * N if per else N
        between = group.S.numpy()[rs.randint(0, group.order, n)].astype(np.float64)
        if group.axis is not None:
            between = between @ z_turns(n, rs)
        R = clustered(centres, n, 15.0, rs, between=between)
        return t(R.reshape(2, N, 3, 3) if per else R).to(dev)

    yield from _fold_outputs("fold_N1027_c4_keep3", ops.sym_fold(hyp(1027, True, c4), c4.to(dev), anchors, 25.0, keep=3))
    yield from _fold_outputs("fold_N1027_axis_no_limit", ops.sym_fold(hyp(1027, False, ax), ax.to(dev), anchors, None))
    R, V = hyp(5, True, c4), vel(5)
    f = ops.sym_fold(R, c4.to(dev), anchors, 25.0, V=V, out=R, V_out=V)
    assert f.R.data_ptr() == R.data_ptr() and f.V.data_ptr() == V.data_ptr()
    yield from _fold_outputs("fold_N5_c4_in_place", f)
    yield from _fold_outputs("fold_N5_axis_V_keep2", ops.sym_fold(hyp(5, False, ax), ax.to(dev), anchors, 40.0, keep=2, V=vel(5)))
    yield from _fold_outputs("fold_N5_axis_no_info", ops.sym_fold(hyp(5, True, ax), ax.to(dev), anchors, 40.0, want_info=False))


def _view_case(rs, B, V, N, per, seed):
    """A (B,V,3,3) Haar, Q: one hypothesis in eight within 20 degrees of a view of sample 0, the others Haar."""
    A = rot.haar_rotations_np(B * V, seed).reshape(B, V, 3, 3)
    n = B * N if per else N
    Q = rot.haar_rotations_np(n, seed + 1)
    near = np.arange(0, n, 8)
    Q[near] = clustered(A[0], len(near), 20.0, rs)
    scores = rs.uniform(-1.0, 1.0, (B, V, N)).astype(np.float32)
    scores[0, V - 1, N // 2], scores[B - 1, 0, N - 1] = np.nan, -np.inf
    return A.astype(np.float32), (Q.reshape(B, N, 3, 3) if per else Q), scores


def _views_family(ops, dev, t):
    import torch
    rs = np.random.RandomState(620)
    weights = lambda V: None if V is None else ([1.5] if V == 1 else [0.0] + [float(x) for x in rs.uniform(0.5, 2.0, V - 1)])
    for N, per in ((5, False), (1027, True)):
        A, Q, _ = _view_case(rs, 2, 3, N, per, 621)
        yield from _entries("views_rotations_N%d" % N, ops.view_rotations(t(Q).to(dev), t(A).to(dev)))
    fuse = [(5, V, limit, given, False) for V in (1, 3, 16) for limit in (True, False) for given in (True, False)]
    fuse += [(1027, 3, True, True, False), (1027, 16, True, False, True), (1027, 1, False, True, False), (1027, 3, False, False, True)]
    for k, (N, V, limit, given, per) in enumerate(fuse):
        A, Q, s = _view_case(rs, 2, V, N, per, 630 + 2 * k)
        want = k % 5 != 4 and k < 14                                         # now and then, and for two of the large cases, the key alone
        fused, key = ops.fuse_view_scores(t(s).to(dev), t(Q).to(dev), t(A).to(dev), weights(V if given else None),
                                          60.0 if limit else None, n_offset=KEY_OFFSET if k % 2 else 0, want_scores=want)
        name = "views_fuse_N%d_V%d_%s_%s" % (N, V, "limit" if limit else "all", "weights" if given else "ones")
        yield from _entries(name + "_key", key)
        if want:
            yield from _entries(name + "_fused", fused)

    A = rot.haar_rotations_np(3 * 5, 680).reshape(3, 5, 3, 3).astype(np.float32)
    A[:, 3] = A[:, 1]                                                        # equal traces: the lower v first
    A[2, 4, 1, 1] = np.nan                                                   # a NaN trace ranks behind every number
    anchor = clustered(A[:, 1], 3, 30.0, rs)
    for K in (1, 5):
        sel = ops.nearest_views(t(anchor).to(dev), t(A).to(dev), K)
        yield from _entries("views_nearest_K%d_idx" % K, sel.idx)
        yield from _entries("views_nearest_K%d_A" % K, sel.A)
    A17 = rot.haar_rotations_np(17 * 4, 681).reshape(17, 4, 3, 3)
    sel = ops.nearest_views(t(rot.haar_rotations_np(17, 682)).to(dev), t(A17).to(dev), 2)     # 17 samples: a second workgroup
    yield from _entries("views_nearest_B17_idx", sel.idx)
    yield from _entries("views_nearest_B17_A", sel.A)

    src = t(rs.normal(size=(2, 3, 1028)).astype(np.float32)).to(dev)         # 257 16-byte words per row: two chunks
    idx = torch.tensor([[2, -1], [0, 1]], dtype=torch.int32, device=dev)     # -1: a row of zeros
    yield from _entries("views_gather", ops.gather_views(src, idx))
    yield from _entries("views_gather_broadcast", ops.gather_views(src[:, 0, :8].contiguous(),
                                                                   torch.zeros((2, 3), dtype=torch.int32, device=dev), broadcast=True))

    compact = [("N1027_counted", 1027, True, None, None), ("N1027_overflow", 1027, False, [0.0, 1.0, 2.0], 16), ("N5_full", 5, True, None, 5)]
    for k, (tag, N, per, w, capacity) in enumerate(compact):
        A, Q, _ = _view_case(rs, 2, 3, N, per, 690 + 2 * k)
        R, slot, counts = ops.view_rotations_compact(t(Q).to(dev), t(A).to(dev), 30.0, w, capacity)
        for what, out in (("R", R), ("slot", slot), ("counts", counts)):
            yield from _entries("views_compact_%s_%s" % (tag, what), out)
        s = t(rs.uniform(-1.0, 1.0, (2, 3, R.shape[2])).astype(np.float32)).to(dev)
        fused, key = ops.fuse_view_scores_compact(s, slot, w, n_offset=KEY_OFFSET, want_scores=capacity != 16)
        if fused is not None:
            yield from _entries("views_compact_%s_fused" % tag, fused)
        yield from _entries("views_compact_%s_key" % tag, key)


def _post_family(ops, dev, t):
    import torch
    rs = np.random.RandomState(640)
    centres = rot.haar_rotations_np(3, 641)
    anchors = np.stack([centres, centres[::-1]]).astype(np.float32)
    anchors[:, 1] = 0.0                                                       # an empty slot
    anchors = t(anchors).to(dev)
    states = {0: [], 3: []}
    for N in (5, 1027, N_PARTS):
        per = N == 1027
        R = clustered(centres, 2 * N if per else N, 25.0, rs)
        R = t(R.reshape(2, N, 3, 3) if per else R).to(dev)
        s = rs.uniform(-0.2, 0.6, (2, N)).astype(np.float32)
        s[0, 1], s[0, N - 1], s[1, N // 2] = np.nan, np.inf, -np.inf           # excluded from the scored set
        cases = [("", s)]
        if N == 1027:
            e = s.copy()
            e[1] = -np.inf                                                     # a sample without a scored hypothesis
            cases.append(("_empty_sample", e))
        for tag, sc in cases:
            for K in (0, 3):
                p = ops.pose_posterior(t(sc).to(dev), R, TEMPERATURE, anchors if K else None, 20.0 if K else None)
                for what, out in zip(p._fields, p):
                    yield from _entries("post_N%d_K%d%s_%s" % (N, K, tag, what), out)
                states[K].append(p.state.clone())
    for K in (0, 3):
        st = torch.stack(states[K])
        merged = ops.merge_posterior(st, K, TEMPERATURE)
        yield from _entries("post_merge_K%d_state" % K, merged)
        carried = ops.merge_posterior(st[1:].contiguous(), K, TEMPERATURE, state=st[0].clone())
        for what, out in zip(ops.PosePosterior._fields, ops.pose_posterior_finish(carried, K, TEMPERATURE)):
            yield from _entries("post_merge_carried_K%d_%s" % (K, what), out)


def _res_family(ops, dev, t):
    rs = np.random.RandomState(650)
    u = t(np.array([0.25, 0.75], np.float32)).to(dev)
    for N in RES_NS:
        s = rs.uniform(-0.2, 0.6, (2, N)).astype(np.float32)
        if N > 1024:
            s[0, 100:900] = -np.inf                                           # a stretch without weight
            s[1, 0:1024] = -50.0                                              # a tile whose fp32 weights underflow
            s[1, 7], s[0, N - 1] = np.nan, np.inf
        s = t(s).to(dev)
        for M in RES_MS:
            idx = ops.resample(s, M, TEMPERATURE, u=u if M == 64 else None)
            yield from _entries("res_N%d_M%d" % (N, M), idx)
            if M == 64 and N in (5, 1027):
                R = t(_per_sample(N, 651) if N == 1027 else rot.haar_rotations_np(N, 651)).to(dev)
                D = t(rot.haar_rotations_np(M, 652)).to(dev)
                yield from _entries("res_N%d_M%d_composed" % (N, M), ops.compose_rotations_indexed(idx, R, D))
    none = t(np.full((2, 5), -np.inf, np.float32)).to(dev)
    yield from _entries("res_no_finite_score", ops.resample(none, 64, TEMPERATURE))


def _asc_family(ops, dev, t):
    rs = np.random.RandomState(660)
    ladder = [0.5]
    for B in (3, 257):
        R = t(rot.haar_rotations_np(B, 661 + B).reshape(B, 1, 3, 3)).to(dev)
        G = rs.normal(size=(B, 1, 3, 3)).astype(np.float32)
        G[1], G[2, 0, 1, 1] = 0.0, np.nan                                     # no direction: every slot is R_cur
        theta = t(rs.uniform(0.01, 0.1, (B, 1)).astype(np.float32)).to(dev)
        cand = ops.so3_ascent_candidates(R, t(G).to(dev), theta, ladder)
        yield from _entries("asc_B%d_candidates" % B, cand)
        cs = rs.uniform(-1.0, 1.0, (B, 2)).astype(np.float32)
        cs[0] = 0.5                                                           # a tie: slot 0 stays
        cs[B - 1, 1] = np.nan
        score = t(cs[:, :1].copy()).to(dev)
        for what, out in zip(("R", "score", "theta"), ops.so3_ascent_select(cand, t(cs).to(dev), ladder, R, score, theta)):
            yield from _entries("asc_B%d_selected_%s" % (B, what), out)


def recompute(ops, dev, family):
    """(name, int32 words) of everything recorded for ``family``, from the library ``ops`` drives."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    families = {"key_": _key_family, "modes_": _modes_family, "fold_": _fold_family, "views_": _views_family,
                "post_": _post_family, "res_": _res_family, "asc_": _asc_family}
    yield from families[family](ops, dev, t)
