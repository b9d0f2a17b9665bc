"""The case table of the C ABI buffer sweep (tests/abi_buffers.py): one row per entry point of _lib.SIGNATURES.

A row is a builder `f(sizes, cu) -> [Case, ...]`: small, non-degenerate inputs as numpy arrays, every pointer's role, dtype
and extent, which *_batch_stride arguments exist and the rule include/ahv.h states for each ('ge': any stride >= the packed
row; 'eq': 0 or exactly the packed row), the alignment the header states, and the call of the ops.py wrapper the baseline
must equal.  `sizes(name, *args)` is the library's own *_workspace_bytes() (a placeholder without the library: the CPU test
only counts pointers).  B = 3 throughout, so that the sample stride shows and rows 1 and 2 start mid-vector.

Alignment, decided by reading the kernels: a pointer is 'refuse' where a kernel reaches it through a reinterpret_cast to a
vector type without testing the address (forward_3d2d's `vol`: float2 in all three kernels; score_features' `f_src` / `f_tgt`:
f32x4; `vol_tgt` of verify_pair and coarse_to_fine: float2 in tgt_regs_load<true> and in forward_3d2d), and 'match' where
the access is scalar or has a scalar fallback (W1 through stage_w1_table and forward_3d2d_small_kernel, the tile loaders of
ahv_tile.h, topk_kernel's shift, the 4-byte loads and stores of the rotate, compose, select and generator kernels).
"""
import importlib
import math
import zlib

import numpy as np
import torch

from . import backward_reference as tb
from . import fused_cases as fc
from . import oplevel_cases as oc
from .abi_buffers import KEY_EMPTY, Case, Host, In, InOut, Null, Out, Sc, Size, Stride, Ws

B = 3
TILE_N = (5, 6, 1025)                 # 5 and 1025: one tile + one, N % 4 = 1, rows 1 and 2 start mid-vector; 6: the LAST row (b = 2)
                                      # starts on a 16-byte boundary and ends two floats into a vector, so a 16-byte store at a ragged
                                      # end lands in the band behind the payload, not in the next sample's row
F32, I64, I32 = np.float32, np.int64, np.int32
RESET = 1                             # AHV_SCORE_RESET_BEST / AHV_SELECT_RESET_KEY / AHV_TOPK_RESET_LIST / AHV_VIEWS_RESET_BEST

EXEMPT = {
    "ahv_abi_version": "no pointer argument",
    "ahv_last_error": "no pointer argument",
    "ahv_device_cu_count": "no pointer argument",
    "ahv_forward_2d3d_workspace_bytes": "size query",
    "ahv_transformer_workspace_bytes": "size query",
    "ahv_score_hypotheses_backward_workspace_bytes": "size query",
    "ahv_topk_workspace_bytes": "size query",
    "ahv_topk_modes_workspace_bytes": "size query",
    "ahv_score_rotation_grad_workspace_bytes": "size query",
    "ahv_pose_posterior_state_bytes": "size query",
    "ahv_pose_posterior_workspace_bytes": "size query",
    "ahv_view_rotations_compact_workspace_bytes": "size query",
    "ahv_resample_workspace_bytes": "size query",
    "ahv_forward_2d3d_f32": "bounds held by tests/test_gpu_encoder_batch.py (guard bands, dirty workspace)",
    "ahv_transformer_blocks_f32": "bounds held by tests/test_gpu_encoder_batch.py (guard bands, dirty workspace)",
}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _rng(*what):
    return np.random.RandomState(zlib.crc32(repr(what).encode()) % (1 << 31))


def haar(n, *what):
    return importlib.import_module("3dahv_amd.rotations").haar_rotations_np(n, zlib.crc32(repr(what).encode()) % (1 << 31))


def randn(shape, *what):
    return _rng(*what).standard_normal(shape).astype(F32)


def unit_features(b, *what):
    f = randn((b, 32, 64), *what)
    return f / np.sqrt((f * f).sum(1, keepdims=True))


def head(*what):
    return [t.numpy() for t in oc.head(zlib.crc32(repr(what).encode()))]


def pack_keys(score, idx):
    """The packed key of include/ahv.h for finite scores."""
    bits = np.asarray(score, F32).view(np.int32).astype(np.int64)
    ordered = np.where(bits >= 0, bits, bits ^ 0x7FFFFFFF)
    return (ordered << 32) | (0xFFFFFFFF - np.asarray(idx, np.int64))


def argmax_keys(scores):
    idx = scores.argmax(1)
    return pack_keys(scores[np.arange(scores.shape[0]), idx], idx)


def topk_lists(scores, k):
    """[B][K] descending distinct keys of a score row (valid lists)."""
    keys = pack_keys(scores, np.arange(scores.shape[1])[None])
    return -np.sort(-keys, axis=1)[:, :k]


def tau(deg):
    return float(np.float32(1.0 + 2.0 * math.cos(math.radians(deg))))


def t5(x, *shape):
    return x.reshape(*shape)


# ---- rows --------------------------------------------------------------------------------------------------------------------
ROWS = {}


def row(entry):
    def deco(f):
        ROWS[entry] = f
        return f
    return deco


def _scorer_shapes(cu):
    return [("N37_no_teams", 37, 4), ("N37", 37, 0), ("N37_split", 37, 2),
            ("round_and_team_tail", fc.sizes(cu, B)["tail_team_first"], 0)]


@row("ahv_score_hypotheses_f32")
def _(sizes, cu):
    out = []
    for name, N, flags in _scorer_shapes(cu):
        W1, W2, b2 = head("score", name)
        out.append(Case("ahv_score_hypotheses_f32", name, [
            In("vol_src", randn((B, 8192), "vs", name)), In("feat_tgt", unit_features(B, "ft", name)),
            In("R", haar(B * N, "R", name), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("n_offset", 0),
            In("W1", W1), In("W2", W2), In("b2", b2), Sc("B", B), Sc("N", N), Out("scores", F32, B * N),
            InOut("best_key", np.full(B, KEY_EMPTY, I64)), Sc("flags", flags)], B, vary=["scores"],
            ops=lambda o, i, N=N, flags=flags: dict(zip(("scores", "best_key"), o.score_hypotheses(
                t5(i["vol_src"], B, 16, 8, 8, 8), t5(i["feat_tgt"], B, 32, 64), t5(i["R"], B, N, 3, 3), i["W1"], i["W2"], i["b2"],
                no_teams=bool(flags & 4), split_f16=bool(flags & 2))))))
    return out


@row("ahv_verify_pair_f32")
def _(sizes, cu):
    out = []
    for name, N, flags in _scorer_shapes(cu):
        W1, W2, b2 = head("verify", name)
        out.append(Case("ahv_verify_pair_f32", name, [
            In("vol_src", randn((B, 8192), "vs", name)), In("vol_tgt", randn((B, 8192), "vt", name), misaligned="refuse"),
            In("R", haar(B * N, "R", name), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("n_offset", 0),
            In("W1", W1), In("W2", W2), In("b2", b2), Sc("B", B), Sc("N", N), Out("scores", F32, B * N),
            InOut("best_key", np.full(B, KEY_EMPTY, I64)), Out("feat_tgt_out", F32, B * 2048), Sc("flags", flags),
            Null("clock_stamps")], B, vary=["scores", "feat_tgt_out"],
            ops=lambda o, i, N=N, flags=flags: dict(zip(("scores", "best_key", "feat_tgt_out"), o.verify_pair(
                t5(i["vol_src"], B, 16, 8, 8, 8), t5(i["vol_tgt"], B, 16, 8, 8, 8), t5(i["R"], B, N, 3, 3), i["W1"], i["W2"], i["b2"],
                no_teams=bool(flags & 4), split_f16=bool(flags & 2), want_feat_tgt=True)))))
    return out


def _score_rows(n, *what):
    """(B, n) distinct finite scores in [-1, 1]."""
    return (_rng(*what).permutation(B * n).reshape(B, n).astype(F32) / F32(B * n) * 2 - 1).astype(F32)


@row("ahv_unpack_best")
def _(sizes, cu):
    s = _score_rows(37, "unpack")
    return [Case("ahv_unpack_best", "B3", [In("best_key", argmax_keys(s), filler=KEY_EMPTY), Sc("B", B), Out("best_score", F32, B),
                                           Out("best_idx", I64, B)], B, vary=["best_score"], distinct=["best_idx"],
                 ops=lambda o, i: dict(zip(("best_score", "best_idx"), o.unpack_best(i["best_key"].reshape(B)))))]


@row("ahv_reset_best")
def _(sizes, cu):
    return [Case("ahv_reset_best", "B3", [Out("best_key", I64, B), Sc("B", B)], B,
                 ops=lambda o, i: {"best_key": o.reset_best(torch.zeros(B, dtype=torch.int64, device=i["_device"]))})]


ROTATE_SHAPES = [("16x8_shared", (16, 8, 8, 8), 5, True), ("16x8_per_hypothesis", (16, 8, 8, 8), 3, False),
                 ("generic", (3, 5, 6, 7), 3, False)]


def _vol5(i, n, shape, shared):
    v = i["vol"].reshape((1 if shared else n,) + shape)
    return v.expand(n, -1, -1, -1, -1) if shared else v


@row("ahv_rotate_volume_f32")
def _(sizes, cu):
    out = []
    for name, shape, n, shared in ROTATE_SHAPES:
        e = int(np.prod(shape))
        out.append(Case("ahv_rotate_volume_f32", name, [
            In("vol", randn((1 if shared else n, e), "vol", name), rows=1 if shared else n, stride="vol_batch_stride"),
            Stride("vol_batch_stride", "ge", shared=shared), In("R", haar(n, "R", name)), Sc("N", n),
            Sc("C", shape[0]), Sc("D", shape[1]), Sc("H", shape[2]), Sc("W", shape[3]), Out("out", F32, n * e)], n, vary=["out"],
            ops=lambda o, i, n=n, shape=shape, shared=shared: {"out": o.rotate_volume(_vol5(i, n, shape, shared), i["R"].reshape(n, 3, 3))}))
    return out


@row("ahv_rotate_volume_backward_f32")
def _(sizes, cu):
    out = []
    for name, shape, n, shared in ROTATE_SHAPES:
        e = int(np.prod(shape))
        R, g = haar(n, "R", name), randn((n, e), "g", name)
        like = torch.zeros((1 if shared else n,) + shape)
        args = (like, torch.from_numpy(R), torch.from_numpy(g).reshape((n,) + shape))
        ref = {}

        def check(got, what, args=args, ref=ref, like=like):
            if not ref:       # the fp64 reference and the fp32 one that measures it, once per case
                ref["r32"], ref["r64"] = oc.ref32("rotate_volume_adjoint", *args), oc.ref64("rotate_volume_adjoint", *args)
            oc.accept(torch.from_numpy(got["grad_vol"].copy()).reshape(like.shape), ref["r32"], ref["r64"], what)

        out.append(Case("ahv_rotate_volume_backward_f32", name, [
            In("grad_out", g), Stride("vol_batch_stride", "ge", shared=shared), In("R", R), Sc("N", n),
            Sc("C", shape[0]), Sc("D", shape[1]), Sc("H", shape[2]), Sc("W", shape[3]),
            Out("grad_vol", F32, e, rows=1 if shared else n, stride="vol_batch_stride")], 1 if shared else n, vary=["grad_vol"] if not shared else [],
            check=check))
    return out


@row("ahv_rotate_volume_rotation_grad_f32")
def _(sizes, cu):
    out = []
    for name, shape, n, shared in ROTATE_SHAPES:
        e = int(np.prod(shape))
        out.append(Case("ahv_rotate_volume_rotation_grad_f32", name, [
            In("grad_out", randn((n, e), "g", name)),
            In("vol", randn((1 if shared else n, e), "vol", name), rows=1 if shared else n, stride="vol_batch_stride"),
            Stride("vol_batch_stride", "ge", shared=shared), In("R", haar(n, "R", name)), Sc("N", n),
            Sc("C", shape[0]), Sc("D", shape[1]), Sc("H", shape[2]), Sc("W", shape[3]), Out("grad_R", F32, n * 9)], n, vary=["grad_R"],
            ops=lambda o, i, n=n, shape=shape, shared=shared: {"grad_R": o.rotate_volume_rotation_grad(
                _vol5(i, n, shape, shared), i["R"].reshape(n, 3, 3), i["grad_out"].reshape((n,) + shape))}))
    return out


@row("ahv_forward_3d2d_f32")
def _(sizes, cu):
    W1, W2, b2 = head("f3d2d")
    return [Case("ahv_forward_3d2d_f32", "M3", [In("vol", randn((B, 8192), "vol"), misaligned="refuse"), In("W1", W1), In("W2", W2),
                                                In("b2", b2), Sc("M", B), Out("out", F32, B * 2048)], B, vary=["out"],
                 ops=lambda o, i: {"out": o.forward_3d2d(t5(i["vol"], B, 16, 8, 8, 8), i["W1"], i["W2"], i["b2"])})]


@row("ahv_score_features_f32")
def _(sizes, cu):
    N = 5
    return [Case("ahv_score_features_f32", "B3_N5", [
        In("f_src", randn((B * N, 2048), "fs"), misaligned="refuse"), In("f_tgt", randn((B, 2048), "ft"), misaligned="refuse"),
        Sc("B", B), Sc("N", N), Out("scores", F32, B * N)], B, vary=["scores"],
        ops=lambda o, i: {"scores": o.score_features(t5(i["f_src"], B, N, 32, 64), t5(i["f_tgt"], B, 32, 64))})]


@row("ahv_argmax_f32")
def _(sizes, cu):
    return [Case("ahv_argmax_f32", "N%d" % N, [In("scores", _score_rows(N, "argmax")), Sc("B", B), Sc("N", N), Sc("n_offset", 0),
                                               InOut("best_key", np.full(B, KEY_EMPTY, I64)), Sc("flags", 0)], B,
                 distinct=["best_key"], ops=lambda o, i, N=N: {"best_key": o.argmax(i["scores"].reshape(B, N), return_key=True)}) for N in TILE_N]


@row("ahv_random_rotations_f32")
def _(sizes, cu):
    N = 1025
    return [Case("ahv_random_rotations_f32", "N1025", [Sc("seed", 7), Sc("offset", 3), Sc("N", N), Out("out", F32, N * 9)], 5,
                 vary=["out"], ops=lambda o, i: {"out": o.random_rotations(N, seed=7, offset=3, device=i["_device"])})]


@row("ahv_so3_grid_f32")
def _(sizes, cu):
    N = 1025
    return [Case("ahv_so3_grid_f32", "N1025", [Sc("n_total", 4096), Sc("offset", 3), Sc("N", N), Out("out", F32, N * 9)], 5,
                 vary=["out"], ops=lambda o, i: {"out": o.so3_grid(4096, i["_device"], offset=3, n=N)})]


@row("ahv_select_rotation_f32")
def _(sizes, cu):
    out = []
    for N in TILE_N:
        for reset in (0, 1):
            keys = argmax_keys(_score_rows(N, "select", N))
            kp = InOut("best_key", keys) if reset else In("best_key", keys, filler=KEY_EMPTY)
            out.append(Case("ahv_select_rotation_f32", "N%d_reset%d" % (N, reset), [
                kp, In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("n_offset", 0),
                Sc("N", N), Sc("B", B), Out("R_out", F32, B * 9), Out("best_score", F32, B), Out("best_idx", I64, B),
                Sc("flags", reset)], B, vary=["R_out", "best_score"], distinct=["best_idx"],
                ops=lambda o, i, N=N, reset=reset: dict(zip(("best_score", "best_idx", "R_out"), o.select_rotation(
                    i["best_key"].reshape(B).clone(), i["R"].reshape(B, N, 3, 3), reset_key=bool(reset))))))
    return out


@row("ahv_compose_rotations_f32")
def _(sizes, cu):
    out = []
    for N in TILE_N:
        N2 = 7
        out.append(Case("ahv_compose_rotations_f32", "N%d" % N, [
            In("best_key", argmax_keys(_score_rows(N, "compose", N)), filler=KEY_EMPTY),
            In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("n_offset", 0), Sc("N", N),
            In("D", haar(N2, "D", N)), Sc("N2", N2), Sc("B", B), Out("out", F32, B * N2 * 9)], B, vary=["out"],
            ops=lambda o, i, N=N, N2=N2: {"out": o.compose_rotations(i["best_key"].reshape(B), i["R"].reshape(B, N, 3, 3),
                                                                     i["D"].reshape(N2, 3, 3))}))
    return out


@row("ahv_topk_f32")
def _(sizes, cu):
    K = 5
    return [Case("ahv_topk_f32", "N%d" % N, [
        In("scores", _score_rows(N, "topk")), Sc("B", B), Sc("N", N), Sc("n_offset", 0), Sc("K", K),
        InOut("keys", np.full(B * K, KEY_EMPTY, I64)), Ws("workspace", sizes("ahv_topk_workspace_bytes", B, N, K), "workspace_bytes", align=8),
        Size("workspace_bytes", "workspace"), Sc("flags", 0)], B, distinct=["keys"],
        ops=lambda o, i, N=N: {"keys": o.topk(i["scores"].reshape(B, N), K)}) for N in TILE_N]


@row("ahv_topk_merge_keys")
def _(sizes, cu):
    P, K = 3, 5
    lists = np.stack([topk_lists(_score_rows(37, "merge", p), K) for p in range(P)])
    return [Case("ahv_topk_merge_keys", "P3_K5", [In("lists", lists, filler=KEY_EMPTY), Sc("P", P), Sc("B", B), Sc("K", K),
                                                  InOut("keys", np.full(B * K, KEY_EMPTY, I64)), Sc("flags", 0)], B,
                 distinct=["keys"], ops=lambda o, i: {"keys": o.merge_topk(i["lists"].reshape(P, B, K))})]


@row("ahv_select_topk_f32")
def _(sizes, cu):
    out, K = [], 5
    for N in TILE_N:
        keys = topk_lists(_score_rows(N, "select_topk", N), K)
        out.append(Case("ahv_select_topk_f32", "N%d" % N, [
            In("keys", keys, filler=KEY_EMPTY), Sc("K", K), In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"),
            Stride("r_batch_stride", "ge"), Sc("n_offset", 0), Sc("N", N), Sc("B", B), Out("R_out", F32, B * K * 9),
            Out("scores_out", F32, B * K), Out("idx_out", I64, B * K), Sc("flags", 0)], B, vary=["R_out", "scores_out"], distinct=["idx_out"],
            ops=lambda o, i, N=N: dict(zip(("scores_out", "idx_out", "R_out"), o.select_topk(i["keys"].reshape(B, K),
                                                                                          i["R"].reshape(B, N, 3, 3))))))
    return out


@row("ahv_compose_rotations_topk_f32")
def _(sizes, cu):
    out, K, N2 = [], 5, 7
    for N in TILE_N:
        out.append(Case("ahv_compose_rotations_topk_f32", "N%d" % N, [
            In("keys", topk_lists(_score_rows(N, "compose_topk", N), K), filler=KEY_EMPTY), Sc("K", K),
            In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("n_offset", 0), Sc("N", N),
            In("D", haar(N2, "D", N)), Sc("N2", N2), Sc("B", B), Out("out", F32, B * K * N2 * 9)], B, vary=["out"],
            ops=lambda o, i, N=N: {"out": o.compose_rotations_topk(i["keys"].reshape(B, K), i["R"].reshape(B, N, 3, 3),
                                                                   i["D"].reshape(N2, 3, 3))}))
    return out


@row("ahv_topk_modes_f32")
def _(sizes, cu):
    K, deg = 4, 30.0
    return [Case("ahv_topk_modes_f32", "N%d" % N, [
        In("scores", _score_rows(N, "modes")), In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"),
        Sc("B", B), Sc("N", N), Sc("n_offset", 0), Sc("K", K), Sc("min_trace", tau(deg)), Out("keys", I64, B * K),
        Ws("workspace", sizes("ahv_topk_modes_workspace_bytes", B, N, K), "workspace_bytes"), Size("workspace_bytes", "workspace")], B, distinct=["keys"],
        ops=lambda o, i, N=N: {"keys": o.topk_modes(i["scores"].reshape(B, N), i["R"].reshape(B, N, 3, 3), K, deg)}) for N in TILE_N]


@row("ahv_view_rotations_f32")
def _(sizes, cu):
    V = 3
    return [Case("ahv_view_rotations_f32", "N%d" % N, [
        In("Q", haar(B * N, "Q", N), rows=B, stride="q_batch_stride"), Stride("q_batch_stride", "eq"), In("A", haar(B * V, "A", N)),
        Sc("B", B), Sc("V", V), Sc("N", N), Out("out", F32, B * V * N * 9)], B, vary=["out"],
        ops=lambda o, i, N=N: {"out": o.view_rotations(i["Q"].reshape(B, N, 3, 3), i["A"].reshape(B, V, 3, 3))}) for N in TILE_N]


@row("ahv_fuse_view_scores_f32")
def _(sizes, cu):
    V, deg, w = 3, 100.0, [1.0, 0.5, 2.0]
    out = []
    for N in TILE_N:
        s = (_rng("fuse", N).permutation(B * V * N).astype(F32) / F32(B * V * N) * 2 - 1).astype(F32)
        out.append(Case("ahv_fuse_view_scores_f32", "N%d" % N, [
            In("scores", s), In("Q", haar(B * N, "Q", N), rows=B, stride="q_batch_stride"), Stride("q_batch_stride", "eq"),
            In("A", haar(B * V, "A", N)), Host("weights", w), Sc("B", B), Sc("V", V), Sc("N", N), Sc("n_offset", 0),
            Sc("min_trace", tau(deg)), Out("fused", F32, B * N), InOut("best_key", np.full(B, KEY_EMPTY, I64)), Sc("flags", 0)], B,
            distinct=["fused", "best_key"],      # (a fused score is -inf where no view is within the angle: not in `vary`)
            ops=lambda o, i, N=N: dict(zip(("fused", "best_key"), o.fuse_view_scores(
                i["scores"].reshape(B, V, N), i["Q"].reshape(B, N, 3, 3), i["A"].reshape(B, V, 3, 3), weights=w, max_view_angle_deg=deg)))))
    return out


@row("ahv_resample_f32")
def _(sizes, cu):
    M = 41
    return [Case("ahv_resample_f32", "N%d" % N, [
        In("scores", _score_rows(N, "resample")), Sc("B", B), Sc("N", N), Sc("beta", 10.0), Sc("M", M),
        In("u", np.array([0.25, 0.5, 0.875], F32)), Out("idx", I64, B * M),
        Ws("workspace", sizes("ahv_resample_workspace_bytes", B, N), "workspace_bytes"), Size("workspace_bytes", "workspace"),
        Sc("flags", 0)], B, distinct=["idx"],
        ops=lambda o, i, N=N: {"idx": o.resample(i["scores"].reshape(B, N), M, temperature=0.1, u=i["u"].reshape(B))}) for N in TILE_N]


@row("ahv_compose_rotations_indexed_f32")
def _(sizes, cu):
    out, M = [], 41
    for N in TILE_N:
        idx = _rng("indexed", N).randint(0, N, (B, M)).astype(I64)
        out.append(Case("ahv_compose_rotations_indexed_f32", "N%d" % N, [
            In("idx", idx, filler=0), In("R", haar(B * N, "R", N), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"),
            Sc("N", N), In("D", haar(M, "D", N)), Sc("M", M), Sc("B", B), Out("out", F32, B * M * 9)], B, vary=["out"],
            ops=lambda o, i, N=N: {"out": o.compose_rotations_indexed(i["idx"].reshape(B, M), i["R"].reshape(B, N, 3, 3),
                                                                      i["D"].reshape(M, 3, 3))}))
    return out


@row("ahv_nearest_views_f32")
def _(sizes, cu):
    V, K = 5, 3
    return [Case("ahv_nearest_views_f32", "V5_K3", [
        In("anchor", haar(B, "anchor")), In("A", haar(B * V, "A")), Sc("B", B), Sc("V", V), Sc("K", K), Out("view_idx", I32, B * K),
        Out("A_sel", F32, B * K * 9)], B, vary=["A_sel"], distinct=["view_idx"],
        ops=lambda o, i: (lambda s: {"view_idx": s.idx, "A_sel": s.A})(
            o.nearest_views(i["anchor"].reshape(B, 3, 3), i["A"].reshape(B, V, 3, 3), K)))]


@row("ahv_gather_views_f32")
def _(sizes, cu):
    V, K, L = 5, 3, 36
    idx = np.array([[4, 0, 2], [1, 1, 3], [0, 4, 2]], I32)
    return [Case("ahv_gather_views_f32", "V5_K3_L36", [
        In("src", randn((B, V * L), "src"), align=16), In("view_idx", idx, filler=0), Sc("B", B), Sc("V", V), Sc("K", K), Sc("L", L),
        Out("dst", F32, B * K * L, align=16), Sc("flags", 0)], B, vary=["dst"],
        ops=lambda o, i: {"dst": o.gather_views(i["src"].reshape(B, V, L), i["view_idx"].reshape(B, K))})]



def _ops():
    return importlib.import_module("3dahv_amd.ops")


# ---- pose posterior ----------------------------------------------------------------------------------------------------------
POST_K, POST_DEG, POST_T = 2, 40.0, 0.1


def _anchors(Rrows, N, K):
    """[B][K] anchors: hypotheses of the set itself, so that the buckets are populated."""
    return np.stack([Rrows.reshape(B, N, 9)[b, [1 + 2 * k for k in range(K)]] for b in range(B)])


@row("ahv_pose_posterior_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for N in TILE_N:
        R = haar(B * N, "R", N)
        nstate = sizes("ahv_pose_posterior_state_bytes", B, POST_K)
        out.append(Case("ahv_pose_posterior_f32", "N%d" % N, [
            In("scores", _score_rows(N, "posterior")), In("R", R, rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"),
            Sc("B", B), Sc("N", N), In("anchors", _anchors(R, N, POST_K)), Sc("K", POST_K), Sc("min_trace", O.min_trace(POST_DEG)),
            Sc("beta", O.inverse_temperature(POST_T)), Out("state", np.uint8, nstate, align=16),
            Ws("workspace", sizes("ahv_pose_posterior_workspace_bytes", B, N, POST_K), "workspace_bytes"),
            Size("workspace_bytes", "workspace"), Sc("flags", 1)], B, distinct=["state"],
            ops=lambda o, i, N=N: {"state": o.pose_posterior(i["scores"].reshape(B, N), i["R"].reshape(B, N, 3, 3), POST_T,
                                                             i["anchors"].reshape(B, POST_K, 3, 3), POST_DEG).state}))
    return out


def _posterior_states(P, *what):
    """[P][B] valid states for K = POST_K, built by the layout of include/ahv.h: a 16-byte header and K + 2 records of 12
    doubles { m, mass, S, M[9] }, each with positive mass and M = mass * c * a rotation, 0.6 <= c < 0.9."""
    rng, rec = _rng(*what), POST_K + 2
    st = np.zeros((P, B, 2 + 12 * rec), np.float64)
    for p in range(P):
        for b in range(B):
            st[p, b, :2].view(np.int64)[:] = (p + b, 0)
            rot = haar(rec, "state", p, b).astype(np.float64).reshape(rec, 9)
            for r in range(rec):
                mass = 0.5 + rng.rand()
                st[p, b, 2 + 12 * r:14 + 12 * r] = np.concatenate([[0.2 + 0.5 * rng.rand(), mass, mass * (0.1 + 0.3 * rng.rand())],
                                                                   mass * (0.6 + 0.3 * rng.rand()) * rot[r]])
    return st.view(np.uint8).reshape(P, B, -1)


@row("ahv_pose_posterior_merge")
def _(sizes, cu):
    P, O = 3, _ops()
    st = _posterior_states(P, "merge")
    return [Case("ahv_pose_posterior_merge", "P3", [
        In("states", st, align=16), Sc("P", P), Sc("B", B), Sc("K", POST_K), Sc("beta", O.inverse_temperature(POST_T)),
        Out("state", np.uint8, st[0].size, align=16), Sc("flags", 1)], B, distinct=["state"],
        ops=lambda o, i: {"state": o.merge_posterior(i["states"].reshape(P, B, -1), POST_K, POST_T)})]


@row("ahv_pose_posterior_finish_f32")
def _(sizes, cu):
    O, K = _ops(), POST_K
    st = _posterior_states(1, "finish")[0]
    names = ("log_z", "entropy", "mean_score", "n_excluded", "mode_prob", "rest_prob", "mode_R_mean", "R_mean", "mode_spread_deg",
             "spread_deg")
    elems = (B, B, B, B, B * K, B, B * K * 9, B * 9, B * K, B)
    return [Case("ahv_pose_posterior_finish_f32", "K2", [
        In("state", st, align=16), Sc("B", B), Sc("K", K), Sc("beta", O.inverse_temperature(POST_T))] +
        [Out(n, I64 if n == "n_excluded" else F32, e) for n, e in zip(names, elems)], B,
        vary=["log_z", "entropy", "mean_score", "mode_prob", "R_mean", "spread_deg"],
        ops=lambda o, i: dict(zip(names, o.pose_posterior_finish(i["state"].reshape(B, -1), K, POST_T)[:10])))]


# ---- compact multi-view ------------------------------------------------------------------------------------------------------
@row("ahv_view_rotations_compact_f32")
def _(sizes, cu):
    out, O, V, deg, w = [], _ops(), 3, 100.0, [1.0, 0.5, 2.0]
    for N in TILE_N:
        cap = N
        out.append(Case("ahv_view_rotations_compact_f32", "N%d" % N, [
            In("Q", haar(B * N, "Q", N), rows=B, stride="q_batch_stride"), Stride("q_batch_stride", "eq"), In("A", haar(B * V, "A", N)),
            Host("weights", w), Sc("B", B), Sc("V", V), Sc("N", N), Sc("min_trace", O.min_trace(deg)), Sc("capacity", cap),
            Out("out", F32, B * V * cap * 9), Out("slot", I32, B * V * N), Out("counts", I64, B * V),
            Ws("workspace", sizes("ahv_view_rotations_compact_workspace_bytes", B, V, N), "workspace_bytes", align=4),
            Size("workspace_bytes", "workspace")], B, vary=["out"], distinct=["slot", "counts"],
            ops=lambda o, i, N=N, cap=cap: dict(zip(("out", "slot", "counts"), o.view_rotations_compact(
                i["Q"].reshape(B, N, 3, 3), i["A"].reshape(B, V, 3, 3), deg, weights=w, capacity=cap)))))
    return out


@row("ahv_fuse_view_scores_compact_f32")
def _(sizes, cu):
    out, V, w = [], 3, [1.0, 0.5, 2.0]
    for N in TILE_N:
        cap = max(2, N // 3)
        rng = _rng("fuse_compact", N)
        slot = np.full((B, V, N), -1, I32)
        for b in range(B):
            for v in range(V):
                take = np.sort(rng.permutation(N)[:min(N, cap + 1)])        # one pair more than the list holds: an overflow
                slot[b, v, take[:cap]] = np.arange(len(take[:cap]))
                slot[b, v, take[cap:]] = -2
        s = (rng.permutation(B * V * cap).astype(F32) / F32(B * V * cap) * 2 - 1).astype(F32)
        out.append(Case("ahv_fuse_view_scores_compact_f32", "N%d" % N, [
            In("scores", s), In("slot", slot, filler=-1), Host("weights", w), Sc("B", B), Sc("V", V), Sc("N", N), Sc("capacity", cap),
            Sc("n_offset", 0), Out("fused", F32, B * N), InOut("best_key", np.full(B, KEY_EMPTY, I64)), Sc("flags", 0)], B,
            distinct=["fused", "best_key"], ops=lambda o, i, N=N, cap=cap: dict(zip(("fused", "best_key"), o.fuse_view_scores_compact(
                i["scores"].reshape(B, V, cap), i["slot"].reshape(B, V, N), weights=w)))))
    return out


# ---- tracking: the predict step, the control record ------------------------------------------------------------------------------
TRACK_M = (37, 257)
SEED, SIGMA, SIGMA_VEL, FRESH, MAX_ANGLE, MAX_SPEED, DAMP = 7, 3.0, 1.0, 3, 10.0, 6.0, 0.75


def _particles(M, *what):
    rng = _rng(*what)
    idx = np.sort(rng.randint(0, M, (B, M)), axis=1).astype(I64)
    key = pack_keys(rng.rand(B).astype(F32), rng.randint(0, M, B))
    return haar(B * M, "R", *what), (0.02 * rng.standard_normal((B, M * 3))).astype(F32), idx, key


@row("ahv_track_advance")
def _(sizes, cu):
    return [Case("ahv_track_advance", "B3", [Sc("seed", SEED), InOut("step", np.array([41], I64)), Sc("B", B), Out("u", F32, B)], B,
                 vary=["u"], ops=lambda o, i: (lambda st: {"u": o.track_advance(st, SEED, B), "step": st})(i["step"].reshape(1).clone()))]


@row("ahv_diffuse_rotations_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for M in TRACK_M:
        R, _, idx, key = _particles(M, "diffuse", M)
        out.append(Case("ahv_diffuse_rotations_f32", "M%d" % M, [
            In("idx", idx, filler=0), In("R", R, rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"), Sc("N", M),
            In("best_key", key, filler=KEY_EMPTY), Sc("M", M), Sc("n_fresh", FRESH), Sc("B", B), Sc("seed", SEED),
            In("step", np.array([41], I64), filler=0), Sc("sigma_rad", O._angle_rad(SIGMA, "sigma")),
            Sc("max_angle_rad", O._angle_rad(MAX_ANGLE, "max_angle")), Out("out", F32, B * M * 9), Out("omega", F32, B * M * 3)], B,
            vary=["out"],
            ops=lambda o, i, M=M: dict(zip(("out", "omega"), o.diffuse_rotations(
                i["R"].reshape(B, M, 3, 3), i["idx"].reshape(B, M), sigma_deg=SIGMA, step=i["step"].reshape(1), seed=SEED,
                best_key=i["best_key"].reshape(B), n_fresh=FRESH, max_angle_deg=MAX_ANGLE, want_omega=True)))))
    return out


def _predict_inputs(M, what):
    R, V, idx, key = _particles(M, what, M)
    return [In("idx", idx, filler=0), In("R", R, rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"),
            In("V", V, rows=B, stride="v_batch_stride"), Stride("v_batch_stride", "eq"), Sc("N", M), In("best_key", key, filler=KEY_EMPTY),
            Sc("M", M)]


@row("ahv_predict_rotations_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for M in TRACK_M:
        out.append(Case("ahv_predict_rotations_f32", "M%d" % M, _predict_inputs(M, "predict") + [
            Sc("n_fresh", FRESH), Sc("B", B), Sc("seed", SEED), In("step", np.array([41], I64), filler=0),
            Sc("sigma_rad", O._angle_rad(SIGMA, "s")), Sc("sigma_vel_rad", O._angle_rad(SIGMA_VEL, "s")), Sc("damping", DAMP),
            Sc("max_angle_rad", O._angle_rad(MAX_ANGLE, "s")), Sc("max_speed_rad", O._angle_rad(MAX_SPEED, "s")), Sc("coast", 1),
            Out("out", F32, B * M * 9), Out("vel_out", F32, B * M * 3), Out("omega", F32, B * M * 3)], B, vary=["out", "vel_out"],
            ops=lambda o, i, M=M: dict(zip(("out", "vel_out", "omega"), o.predict_rotations(
                i["R"].reshape(B, M, 3, 3), i["V"].reshape(B, M, 3), i["idx"].reshape(B, M), sigma_deg=SIGMA, sigma_vel_deg=SIGMA_VEL,
                damping=DAMP, step=i["step"].reshape(1), seed=SEED, best_key=i["best_key"].reshape(B), coast=True, n_fresh=FRESH,
                max_angle_deg=MAX_ANGLE, max_speed_deg=MAX_SPEED, want_omega=True)))))
    return out


def _control(O):
    return O.track_control_state(B, SIGMA, SIGMA_VEL, FRESH, "cpu").numpy()


@row("ahv_predict_rotations_ctl_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for M in TRACK_M:
        out.append(Case("ahv_predict_rotations_ctl_f32", "M%d" % M, _predict_inputs(M, "predict_ctl") + [
            In("control", _control(O), filler=0), Sc("B", B), Sc("seed", SEED), In("step", np.array([41], I64), filler=0),
            Sc("damping", DAMP), Sc("max_angle_rad", O._angle_rad(MAX_ANGLE, "s")), Sc("max_speed_rad", O._angle_rad(MAX_SPEED, "s")),
            Sc("coast", 1), Out("out", F32, B * M * 9), Out("vel_out", F32, B * M * 3), Out("omega", F32, B * M * 3)], B,
            vary=["out", "vel_out"],
            ops=lambda o, i, M=M: dict(zip(("out", "vel_out", "omega"), o.predict_rotations_controlled(
                i["R"].reshape(B, M, 3, 3), i["control"].reshape(B, 8), i["V"].reshape(B, M, 3), i["idx"].reshape(B, M), damping=DAMP,
                step=i["step"].reshape(1), seed=SEED, best_key=i["best_key"].reshape(B), coast=True, max_angle_deg=MAX_ANGLE,
                max_speed_deg=MAX_SPEED, want_omega=True)))))
    return out


@row("ahv_track_control_f32")
def _(sizes, cu):
    out, O = [], _ops()
    kw = dict(first=2, sigma_deg=SIGMA, sigma_vel_deg=SIGMA_VEL, n_fresh=FRESH, sigma_min_deg=0.5, sigma_max_deg=8.0, gain=1.5, rate=0.5,
              score_floor=0.1, n_fresh_lost=5)
    for M in TRACK_M:
        R, V, _, _ = _particles(M, "control", M)
        first, s0, sv0, nf, smin, smax, gain, rate, floor, nlost = O._control_params(
            kw["first"], SIGMA, SIGMA_VEL, FRESH, 0.5, 8.0, 1.5, 0.5, 0.1, 5, M)
        out.append(Case("ahv_track_control_f32", "M%d" % M, [
            In("R_cur", R), In("V_cur", V), In("idx", np.array([5, M - 1, 0], I64), filler=0), In("score", np.array([0.6, 0.4, 0.05], F32)),
            Sc("B", B), Sc("M", M), Sc("first", first), Sc("sigma0_rad", s0), Sc("sigma_vel0_rad", sv0), Sc("n_fresh0", nf),
            Sc("sigma_min_rad", smin), Sc("sigma_max_rad", smax), Sc("gain", gain), Sc("rate", rate), Sc("score_floor", floor),
            Sc("n_fresh_lost", nlost), InOut("control", _control(O)), Out("reacquired", np.uint8, B)], B, distinct=["control", "reacquired"],
            ops=lambda o, i, M=M: (lambda c: {"reacquired": o.track_control(c, i["R_cur"].reshape(B, M, 3, 3), i["idx"].reshape(B),
                                                                           i["score"].reshape(B), i["V_cur"].reshape(B, M, 3), **kw)
                                              .view(torch.uint8), "control": c})(i["control"].reshape(B, 8).clone())))
    return out



# ---- tracking: the smoothers over a ring of H = 3 frames ------------------------------------------------------------------------
RING_H, RING_T, SMOOTH_SIGMA, SMOOTH_JUMP = 3, 41, 4.0, 8.0       # frame 41 lives in slot 2, its predecessors in slot 1


def _ring(M, *what):
    """A recorded ring: hist_R / hist_P [H][B][M] rotations, finite deltas, back-pointers inside [0, M), alpha and emit."""
    rng = _rng(*what)
    n = RING_H * B * M
    return dict(hist_R=haar(n, "hR", *what), hist_P=haar(n, "hP", *what), hist_delta=rng.standard_normal(n).astype(F32),
                hist_back=rng.randint(0, M, n).astype(I32), hist_alpha=rng.standard_normal(n).astype(F32),
                hist_emit=rng.standard_normal(n).astype(F32), R_cur=haar(B * M, "cur", *what),
                scores=_score_rows(M, "ring", *what), V_cur=(0.02 * rng.standard_normal(B * M * 3)).astype(F32),
                step=np.array([RING_T], I64))


def _history(o, i, M):
    h = lambda k, *shape: i[k].reshape(RING_H, B, M, *shape).clone()
    return o.SmoothHistory(h("hist_R", 3, 3), h("hist_P", 3, 3), h("hist_delta"), h("hist_back"))


def _smooth_step_ops(o, i, M):
    h = o.smooth_step(_history(o, i, M), i["R_cur"].reshape(B, M, 3, 3), i["scores"].reshape(B, M), i["step"].reshape(1), POST_T,
                      SMOOTH_SIGMA, SMOOTH_JUMP, V=i["V_cur"].reshape(B, M, 3), damping=DAMP)
    return {"hist_R": h.R, "hist_P": h.P, "hist_delta": h.delta, "hist_back": h.back}


@row("ahv_smooth_step_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for M in TRACK_M:
        r = _ring(M, "smooth_step", M)
        out.append(Case("ahv_smooth_step_f32", "M%d" % M, [
            In("R_cur", r["R_cur"]), In("scores", r["scores"]), In("V_cur", r["V_cur"]), In("step", r["step"], filler=0), Sc("first_step", 1),
            Sc("B", B), Sc("M", M), Sc("H", RING_H), Sc("beta", O.inverse_temperature(POST_T)), Sc("sigma_rad", O._angle_rad(SMOOTH_SIGMA, "s")),
            Sc("jump", SMOOTH_JUMP), Sc("damping", DAMP), InOut("hist_R", r["hist_R"]), InOut("hist_P", r["hist_P"]),
            InOut("hist_delta", r["hist_delta"]), InOut("hist_back", r["hist_back"])], B,
            vary=["hist_R", "hist_P", "hist_delta"], distinct=["hist_back"],
            ops=lambda o, i, M=M: _smooth_step_ops(o, i, M)))
    return out


@row("ahv_smooth_backtrace_f32")
def _(sizes, cu):
    out, F = [], RING_H
    for M in TRACK_M:
        r = _ring(M, "backtrace", M)
        out.append(Case("ahv_smooth_backtrace_f32", "M%d" % M, [
            In("hist_R", r["hist_R"]), In("hist_delta", r["hist_delta"]), In("hist_back", r["hist_back"], filler=0),
            In("step", r["step"], filler=0), Sc("first_step", 1), Sc("B", B), Sc("M", M), Sc("H", RING_H), Sc("F", F),
            Out("path_idx", I64, B * F), Out("path_R", F32, B * F * 9)], B, vary=["path_R"], distinct=["path_idx"],
            ops=lambda o, i, M=M: (lambda p: {"path_idx": p.idx, "path_R": p.R})(
                o.smooth_backtrace(_history(o, dict(i, hist_P=i["hist_R"]), M), i["step"].reshape(1)))))
    return out


@row("ahv_marginal_step_f32")
def _(sizes, cu):
    out, O = [], _ops()
    for M in TRACK_M:
        r = _ring(M, "marginal_step", M)
        out.append(Case("ahv_marginal_step_f32", "M%d" % M, [
            In("R_cur", r["R_cur"]), In("scores", r["scores"]), In("step", r["step"], filler=0), Sc("first_step", 1), Sc("B", B), Sc("M", M),
            Sc("H", RING_H), Sc("beta", O.inverse_temperature(POST_T)), Sc("sigma_rad", O._angle_rad(SMOOTH_SIGMA, "s")),
            Sc("jump", SMOOTH_JUMP), In("hist_R", r["hist_R"]), In("hist_P", r["hist_P"]), InOut("hist_alpha", r["hist_alpha"]),
            InOut("hist_emit", r["hist_emit"])], B, vary=["hist_alpha", "hist_emit"],
            ops=lambda o, i, M=M: (lambda m: {"hist_alpha": m.alpha, "hist_emit": m.emit})(o.marginal_step(
                _history(o, dict(i, hist_delta=i["hist_alpha"], hist_back=torch.zeros(RING_H * B * M, dtype=torch.int32, device=i["_device"])), M),
                o.MarginalHistory(i["hist_alpha"].reshape(RING_H, B, M).clone(), i["hist_emit"].reshape(RING_H, B, M).clone()),
                i["R_cur"].reshape(B, M, 3, 3), i["scores"].reshape(B, M), i["step"].reshape(1), POST_T, SMOOTH_SIGMA, SMOOTH_JUMP))))
    return out


@row("ahv_marginal_smooth_f32")
def _(sizes, cu):
    out, O, F = [], _ops(), RING_H
    for M in TRACK_M:
        r = _ring(M, "marginal_smooth", M)
        out.append(Case("ahv_marginal_smooth_f32", "M%d" % M, [
            In("hist_R", r["hist_R"]), In("hist_P", r["hist_P"]), In("hist_alpha", r["hist_alpha"]), In("hist_emit", r["hist_emit"]),
            In("step", r["step"], filler=0), Sc("first_step", 1), Sc("B", B), Sc("M", M), Sc("H", RING_H), Sc("F", F),
            Sc("sigma_rad", O._angle_rad(SMOOTH_SIGMA, "s")), Sc("jump", SMOOTH_JUMP), Out("logw", F32, B * F * M), Out("idx", I64, B * F),
            Out("R", F32, B * F * 9)], B, vary=["logw", "R"], distinct=["idx"],
            ops=lambda o, i, M=M: dict(zip(("logw", "idx", "R"), o.marginal_smooth(
                _history(o, dict(i, hist_delta=i["hist_alpha"], hist_back=torch.zeros(RING_H * B * M, dtype=torch.int32, device=i["_device"])), M),
                o.MarginalHistory(i["hist_alpha"].reshape(RING_H, B, M), i["hist_emit"].reshape(RING_H, B, M)),
                i["step"].reshape(1), SMOOTH_SIGMA, SMOOTH_JUMP)))))
    return out



# ---- joint pose inference: V = 5 nodes, every ordered pair an edge (E = 20, D = 8), N = 65 candidates ----------------------------
GRAPH_V, GRAPH_K, GRAPH_N, GRAPH_FRESH, GRAPH_SIGMA = 5, 2, 65, 4, 5.0


def _graph(what):
    topo = _ops().PoseGraphTopology(GRAPH_V)
    E, k = topo.n_edges, GRAPH_K
    D = topo.degree[k]
    return dict(E=E, D=D, edges=topo.edges_dev.numpy().astype(I32), pair_R=haar(B * E, "pair", what),
                incident=topo.incident_dev.numpy()[topo.offset[k]:topo.offset[k] + D].astype(I32),
                pair_score=(_rng("pscore", what).permutation(B * E).astype(F32) / F32(B * E)).astype(F32), A=haar(B * GRAPH_V, "A", what))


@row("ahv_pose_graph_init_f32")
def _(sizes, cu):
    g, V = _graph("init"), GRAPH_V
    return [Case("ahv_pose_graph_init_f32", "V5", [
        In("pair_R", g["pair_R"]), In("pair_score", g["pair_score"]), In("edges", g["edges"], filler=0), Sc("B", B), Sc("V", V),
        Sc("E", g["E"]), Sc("root", 1), Out("A", F32, B * V * 9), Out("parent_edge", I32, B * V), Out("reached", I32, B * V)], B, vary=["A"], distinct=["parent_edge"],
        ops=lambda o, i: dict(zip(("A", "parent_edge", "reached"), o.pose_graph_init(
            i["pair_R"].reshape(B, g["E"], 3, 3), i["pair_score"].reshape(B, g["E"]), o.PoseGraphTopology(V, root=1, device=i["_device"])))))]


@row("ahv_pose_graph_propose_f32")
def _(sizes, cu):
    g, V, N, O = _graph("propose"), GRAPH_V, GRAPH_N, _ops()
    return [Case("ahv_pose_graph_propose_f32", "V5_D8_N65", [
        In("A", g["A"]), In("pair_R", g["pair_R"]), In("pair_score", g["pair_score"]), In("edges", g["edges"], filler=0),
        In("incident", g["incident"], filler=0), Sc("B", B), Sc("V", V), Sc("E", g["E"]), Sc("k", GRAPH_K), Sc("D", g["D"]), Sc("N", N),
        Sc("n_fresh", GRAPH_FRESH), Sc("seed", SEED), In("counter", np.array([41], I64), filler=0), Sc("sweep", 2),
        Sc("sigma_rad", O._angle_rad(GRAPH_SIGMA, "s")), Out("Q", F32, B * N * 9), Out("Rrel", F32, B * g["D"] * N * 9)], B,
        vary=["Q", "Rrel"],
        ops=lambda o, i: dict(zip(("Q", "Rrel"), o.pose_graph_propose(
            i["A"].reshape(B, V, 3, 3), i["pair_R"].reshape(B, g["E"], 3, 3), i["pair_score"].reshape(B, g["E"]),
            o.PoseGraphTopology(V, device=i["_device"]), GRAPH_K, N, GRAPH_SIGMA, sweep=2, seed=SEED, counter=i["counter"].reshape(1),
            n_fresh=GRAPH_FRESH))))]


@row("ahv_pose_graph_commit_f32")
def _(sizes, cu):
    V, N = GRAPH_V, GRAPH_N
    rng = _rng("commit")
    key = pack_keys(rng.rand(B).astype(F32), rng.randint(0, N, B))
    return [Case("ahv_pose_graph_commit_f32", "V5_N65", [
        In("key", key, filler=KEY_EMPTY), In("Q", haar(B * N, "Q", "commit")), Sc("B", B), Sc("V", V), Sc("k", GRAPH_K), Sc("N", N),
        InOut("A", haar(B * V, "A", "commit")), InOut("node_score", rng.rand(B * V).astype(F32))], B, vary=["A", "node_score"],
        ops=lambda o, i: dict(zip(("A", "node_score"), o.pose_graph_commit(
            i["key"].reshape(B), i["Q"].reshape(B, N, 3, 3), i["A"].reshape(B, V, 3, 3).clone(), i["node_score"].reshape(B, V).clone(),
            GRAPH_K))))]


# ---- SO(3) ascent -------------------------------------------------------------------------------------------------------------
ASCENT_K, LADDER = 5, [0.5, 1.0, 2.0]


@row("ahv_so3_ascent_candidates_f32")
def _(sizes, cu):
    K, L = ASCENT_K, len(LADDER)
    return [Case("ahv_so3_ascent_candidates_f32", "K5_L3", [
        In("R_cur", haar(B * K, "cur")), In("grad_R", randn((B * K, 9), "grad")), In("theta", (0.05 + 0.1 * _rng("th").rand(B * K)).astype(F32)),
        In("ladder", np.array(LADDER, F32)), Sc("L", L), Sc("B", B), Sc("K", K), Out("R_cand", F32, B * K * (L + 1) * 9)], B, vary=["R_cand"],
        ops=lambda o, i: {"R_cand": o.so3_ascent_candidates(i["R_cur"].reshape(B, K, 3, 3), i["grad_R"].reshape(B, K, 3, 3),
                                                            i["theta"].reshape(B, K), LADDER)})]


@row("ahv_so3_ascent_select_f32")
def _(sizes, cu):
    K, L = ASCENT_K, len(LADDER)
    n = K * (L + 1)
    return [Case("ahv_so3_ascent_select_f32", "K5_L3", [
        In("R_cand", haar(B * n, "cand")), In("cand_scores", _score_rows(n, "cand")), In("ladder", np.array(LADDER, F32)), Sc("L", L),
        Sc("B", B), Sc("K", K), InOut("R_cur", haar(B * K, "cur2")), InOut("score_cur", _score_rows(K, "cur")),
        InOut("theta", (0.05 + 0.1 * _rng("th2").rand(B * K)).astype(F32))], B, vary=["R_cur", "score_cur", "theta"],
        ops=lambda o, i: dict(zip(("R_cur", "score_cur", "theta"), o.so3_ascent_select(
            i["R_cand"].reshape(B, n, 3, 3), i["cand_scores"].reshape(B, n), LADDER, i["R_cur"].reshape(B, K, 3, 3).clone(),
            i["score_cur"].reshape(B, K).clone(), i["theta"].reshape(B, K).clone()))))]


# ---- training: backward, training forward, rotation gradient ---------------------------------------------------------------------
TRAIN_SHAPES = ((3, 9), (2, 130))
GRADS = ("grad_vol_src", "grad_feat_tgt", "grad_W1", "grad_W2", "grad_b2")


def _train_inputs(what, b, n):
    g = np.load(oc.GOLDEN + "/score_n128.npz", allow_pickle=False)        # the head of tests/test_gpu_backward.py::make_case
    return dict(vol_src=(1.1 * randn((b, 8192), "vs", what, b, n)).astype(F32), feat_tgt=unit_features(b, "ft", what, b, n),
                R=haar(b * n, "R", what, b, n), W1=np.ascontiguousarray(g["W1"]).reshape(32, 384), W2=np.ascontiguousarray(g["W2"]).reshape(32, 32),
                b2=np.ascontiguousarray(g["b2"]), grad_scores=randn((b, n), "gs", what, b, n))


def _train_head(x, b, n, rule="eq"):
    return [In("vol_src", x["vol_src"]), In("feat_tgt", x["feat_tgt"]), In("R", x["R"], rows=b, stride="r_batch_stride"),
            Stride("r_batch_stride", rule), In("W1", x["W1"]), In("W2", x["W2"]), In("b2", x["b2"]), Sc("B", b), Sc("N", n)]


def _train_tensors(i, b, n):
    return (i["vol_src"].reshape(b, 16, 8, 8, 8), i["feat_tgt"].reshape(b, 32, 64), i["R"].reshape(b, n, 3, 3), i["W1"], i["W2"], i["b2"])


def _grad_check(x, b, n):
    """Every variant against the kink-aware fp64 autograd reference of tests/backward_reference.py at its GRAD_RTOL."""
    ref = {}

    def check(got, what):
        if not ref:
            t = lambda a, *shape: torch.from_numpy(a).reshape(*shape)
            ref["k"] = tb.KinkReference(t(x["vol_src"], b, 16, 8, 8, 8), t(x["feat_tgt"], b, 32, 64), t(x["R"], b, n, 3, 3), t(x["W1"], 32, 384),
                                        t(x["W2"], 32, 32), t(x["b2"], 32), t(x["grad_scores"], b, n))
        shapes = ((b, 16, 8, 8, 8), (b, 32, 64), (32, 384), (32, 32), (32,))
        errs, n_amb, _ = ref["k"].errors([torch.from_numpy(got[k].copy()).reshape(s) for k, s in zip(GRADS, shapes)])
        assert all(e < tb.GRAD_RTOL for e in errs), (what, errs, n_amb)       # (all: a NaN error is no pass)
    return check


def _backward_case(entry, sizes, b, n, saved):
    x = _train_inputs("backward", b, n)
    nbytes = sizes("ahv_score_hypotheses_backward_workspace_bytes", b, n)
    if saved:          # the workspace is a state: what the training forward left for the same inputs
        ws = np.zeros(nbytes, np.uint8)
        if getattr(sizes, "live", False):
            t = lambda a, *shape: torch.from_numpy(a).reshape(*shape).cuda()
            ws = _ops().score_hypotheses_train(t(x["vol_src"], b, 16, 8, 8, 8), t(x["feat_tgt"], b, 32, 64), t(x["R"], b, n, 3, 3),
                                               t(x["W1"], 32, 384), t(x["W2"], 32, 32), t(x["b2"], 32))[1].cpu().numpy().view(np.uint8)[:nbytes]
        wsp = InOut("workspace", ws, align=16)
    else:
        wsp = Ws("workspace", nbytes, "workspace_bytes")
    return Case(entry, "B%d_N%d" % (b, n), _train_head(x, b, n) + [
        In("grad_scores", x["grad_scores"]), wsp, Size("workspace_bytes", "workspace"), Out("grad_vol_src", F32, b * 8192),
        Out("grad_feat_tgt", F32, b * 2048), Out("grad_W1", F32, 32 * 384), Out("grad_W2", F32, 32 * 32), Out("grad_b2", F32, 32)], b,
        vary=["grad_vol_src", "grad_feat_tgt"], check=_grad_check(x, b, n))


@row("ahv_score_hypotheses_backward_f32")
def _(sizes, cu):
    return [_backward_case("ahv_score_hypotheses_backward_f32", sizes, b, n, False) for b, n in TRAIN_SHAPES]


@row("ahv_score_hypotheses_backward_saved_f32")
def _(sizes, cu):
    return [_backward_case("ahv_score_hypotheses_backward_saved_f32", sizes, b, n, True) for b, n in TRAIN_SHAPES]


@row("ahv_score_hypotheses_train_f32")
def _(sizes, cu):
    out = []
    for b, n in TRAIN_SHAPES:
        x = _train_inputs("train", b, n)
        out.append(Case("ahv_score_hypotheses_train_f32", "B%d_N%d" % (b, n), _train_head(x, b, n) + [
            Out("scores", F32, b * n), Ws("workspace", sizes("ahv_score_hypotheses_backward_workspace_bytes", b, n), "workspace_bytes"),
            Size("workspace_bytes", "workspace")], b, vary=["scores"],
            ops=lambda o, i, b=b, n=n: {"scores": o.score_hypotheses_train(*_train_tensors(i, b, n))[0]}))
    return out


@row("ahv_score_rotation_grad_f32")
def _(sizes, cu):
    out = []
    for b, n in TRAIN_SHAPES:
        x = _train_inputs("rotation_grad", b, n)
        out.append(Case("ahv_score_rotation_grad_f32", "B%d_N%d" % (b, n), _train_head(x, b, n) + [
            In("grad_scores", x["grad_scores"]), Ws("workspace", sizes("ahv_score_rotation_grad_workspace_bytes", b, n), "workspace_bytes"),
            Size("workspace_bytes", "workspace"), Out("grad_R", F32, b * n * 9)], b, vary=["grad_R"],
            ops=lambda o, i, b=b, n=n: {"grad_R": o.score_rotation_grad(*_train_tensors(i, b, n), grad_scores=i["grad_scores"].reshape(b, n))}))
    return out


# ---- symmetry ---------------------------------------------------------------------------------------------------------------------
SYM_G = 2


def _sym_group():
    """Per sample: C2 about the z axis of the source view's frame, S[0] the identity exactly, and z as the continuous axis
    (both members map it to itself)."""
    S = np.tile(np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])]).astype(F32).reshape(1, SYM_G * 9), (B, 1))
    return S, np.tile(np.array([0, 0, 1], F32), (B, 1))


def _sym_inputs():
    S, axis = _sym_group()
    return [In("S", S, rows=B, stride="s_batch_stride"), Stride("s_batch_stride", "eq"), Sc("G", SYM_G),
            In("axis", axis, rows=B, stride="axis_batch_stride"), Stride("axis_batch_stride", "eq")]


def _symmetry(i):
    import types
    return types.SimpleNamespace(S=i["S"].reshape(B, SYM_G, 3, 3), axis=i["axis"].reshape(B, 3))


@row("ahv_topk_modes_sym_f32")
def _(sizes, cu):
    K, deg, O = 4, 30.0, _ops()
    return [Case("ahv_topk_modes_sym_f32", "N%d" % N, [
        In("scores", _score_rows(N, "modes_sym")), In("R", haar(B * N, "R", "sym", N), rows=B, stride="r_batch_stride"),
        Stride("r_batch_stride", "eq"), Sc("B", B), Sc("N", N), Sc("n_offset", 0), Sc("K", K), Sc("min_trace", O.min_trace(deg))] + _sym_inputs() + [
        Out("keys", I64, B * K), Ws("workspace", sizes("ahv_topk_modes_workspace_bytes", B, N, K), "workspace_bytes"),
        Size("workspace_bytes", "workspace")], B, distinct=["keys"],
        ops=lambda o, i, N=N: {"keys": o.topk_modes(i["scores"].reshape(B, N), i["R"].reshape(B, N, 3, 3), K, deg, symmetry=_symmetry(i))})
        for N in TILE_N]


@row("ahv_sym_fold_f32")
def _(sizes, cu):
    out, K, deg, keep, O = [], 2, 60.0, 1, _ops()
    for N in TILE_N:
        R = haar(B * N, "R", "fold", N)
        out.append(Case("ahv_sym_fold_f32", "N%d" % N, [In("R", R, rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "eq"),
                                                       Sc("B", B), Sc("N", N)] + _sym_inputs() + [
            In("anchors", _anchors(R, N, K)), Sc("K", K), Sc("min_trace", O.min_trace(deg)), Sc("keep", keep),
            In("V", (0.02 * randn((B, N * 3), "V", N)).astype(F32)), Out("R_out", F32, B * N * 9), Out("V_out", F32, B * N * 3),
            Out("which", I32, B * N), Out("elem", I32, B * N), Out("trace", F32, B * N)], B, vary=["R_out", "V_out"],
            distinct=["which", "elem", "trace"],
            ops=lambda o, i, N=N: dict(zip(("R_out", "which", "elem", "trace", "V_out"), o.sym_fold(
                i["R"].reshape(B, N, 3, 3), _symmetry(i), i["anchors"].reshape(B, K, 3, 3), deg, keep, V=i["V"].reshape(B, N, 3))))))
    return out


# ---- coarse to fine ---------------------------------------------------------------------------------------------------------------
@row("ahv_coarse_to_fine_f32")
def _(sizes, cu):
    out = []
    tail = fc.c2f_sizes(cu, B)           # stage 0: a round + one hypothesis by a team; stage 1: a round + a team tail of three
    for name, flags, (N, N2) in (("N37_no_teams", 4, (37, 11)), ("N37", 0, (37, 11)), ("round_and_team_tail", 0, tail)):
        W1, W2, b2 = head("c2f", name)
        out.append(Case("ahv_coarse_to_fine_f32", name, [
            In("vol_src", randn((B, 8192), "vs", name)), In("vol_tgt", randn((B, 8192), "vt", name), misaligned="refuse"),
            In("R", haar(B * N, "R", name), rows=B, stride="r_batch_stride"), Stride("r_batch_stride", "ge"), Sc("N", N),
            In("D", haar(N2, "D", name)), Sc("N2", N2), In("W1", W1), In("W2", W2), In("b2", b2), Sc("B", B),
            Out("scores_coarse", F32, B * N), Out("scores_fine", F32, B * N2), InOut("keys", np.full(2 * B, KEY_EMPTY, I64)),
            InOut("sync", np.zeros(2 * B + 1, np.uint32)), Out("feat_tgt_out", F32, B * 2048), Out("R_pred", F32, B * 9),
            Out("fine_score", F32, B), Out("fine_idx", I64, B), Out("coarse_score", F32, B), Out("coarse_idx", I64, B), Sc("flags", flags)], B,
            vary=["scores_coarse", "scores_fine", "R_pred", "fine_score", "coarse_score"], distinct=["fine_idx", "coarse_idx"],
            ops=lambda o, i, flags=flags, N=N, N2=N2: (lambda r: {"scores_coarse": r["coarse_scores"], "scores_fine": r["fine_scores"],
                                                      "feat_tgt_out": r["feat_tgt"], "R_pred": r["R_pred"], "fine_score": r["fine_score"],
                                                      "fine_idx": r["fine_idx"], "coarse_score": r["coarse_score"],
                                                      "coarse_idx": r["coarse_idx"], "keys": r["state"].keys, "sync": r["state"].sync})(
                o.coarse_to_fine(i["vol_src"].reshape(B, 16, 8, 8, 8), i["vol_tgt"].reshape(B, 16, 8, 8, 8), i["R"].reshape(B, N, 3, 3),
                                 i["D"].reshape(N2, 3, 3), i["W1"], i["W2"], i["b2"], want_scores=True, want_feat_tgt=True,
                                 no_teams=bool(flags & 4)))))
    return out


def cases(entry, sizes=None, cu=oc.CU_MI355X):
    return ROWS[entry](sizes or (lambda name, *a: 64), cu)
