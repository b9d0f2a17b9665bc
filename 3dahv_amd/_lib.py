"""ctypes binding of libahv_hip.so (the C ABI in include/ahv.h).

There is no CPU fallback: if the library is missing or a call fails, an
exception is raised.  ``build()`` compiles it with hipcc for gfx950 (works
without a GPU: hipcc cross-compiles).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libahv_hip.so")

AHV_SCORE_RESET_BEST = 1
AHV_SCORE_SPLIT_F16 = 2
AHV_SCORE_NO_TEAMS = 4
AHV_SCORE_SPARE_CUS_SHIFT = 8
AHV_SELECT_RESET_KEY = 1
AHV_KEY_EMPTY = -(1 << 63)
AHV_TOPK_MAX_K = 64
AHV_TOPK_RESET_LIST = 1
AHV_SO3_MAX_LADDER = 8
AHV_POSTERIOR_MAX_MODES = 16
AHV_POSTERIOR_RESET_STATE = 1
AHV_VIEWS_MAX = 16
AHV_SYM_MAX_ELEMENTS = 64
AHV_SYM_FOLD_MAX_ANCHORS = 16
AHV_VIEWS_RESET_BEST = 1
AHV_VIEWS_NO_ANGLE_LIMIT = 2
AHV_VIEW_SLOT_EXCLUDED = -1
AHV_VIEW_SLOT_OVERFLOW = -2
AHV_GATHER_BROADCAST = 1
AHV_TRACK_CONTROL_WORDS = 8
AHV_GRAPH_MAX_NODES = 16
AHV_GRAPH_MAX_EDGES = 256
AHV_GRAPH_EDGE_OUTGOING = 1 << 30
AHV_TRACK_LOST, AHV_TRACK_REACQUIRED, AHV_TRACK_UPDATED = 1, 2, 4

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_u32 = ctypes.c_uint

# name -> (restype, argtypes); mirrors include/ahv.h declaration by declaration
SIGNATURES = {
    "ahv_abi_version": (_int, []),
    "ahv_last_error": (ctypes.c_char_p, []),
    "ahv_device_cu_count": (_int, []),
    "ahv_score_hypotheses_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp, _u32, _vp]),
    "ahv_score_hypotheses_clocked_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp, _u32,
                                                _vp, _vp]),
    "ahv_verify_pair_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp, _vp, _u32, _vp, _vp]),
    "ahv_unpack_best": (_int, [_vp, _int, _vp, _vp, _vp]),
    "ahv_reset_best": (_int, [_vp, _int, _vp]),
    "ahv_rotate_volume_f32": (_int, [_vp, _i64, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    "ahv_rotate_volume_backward_f32": (_int, [_vp, _i64, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    # (grad_out, vol, vol_batch_stride, R, N, C, D, H, W, grad_R, stream)
    "ahv_rotate_volume_rotation_grad_f32": (_int, [_vp, _vp, _i64, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    "ahv_forward_3d2d_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "ahv_score_features_f32": (_int, [_vp, _vp, _int, _i64, _vp, _vp]),
    "ahv_argmax_f32": (_int, [_vp, _int, _i64, _i64, _vp, _u32, _vp]),
    "ahv_random_rotations_f32": (_int, [ctypes.c_uint64, ctypes.c_uint64, _i64, _vp, _vp]),
    "ahv_so3_grid_f32": (_int, [_i64, _i64, _i64, _vp, _vp]),
    "ahv_select_rotation_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _u32, _vp]),
    "ahv_compose_rotations_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _int, _vp, _vp]),
    "ahv_coarse_to_fine_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
}

class BlockWeights(ctypes.Structure):
    """Mirror of ``ahv_block_weights`` (include/ahv.h)."""
    _fields_ = [(n, _vp) for n in ("w_qkv", "w_out", "b_out", "ln1_g", "ln1_b", "w_ff1", "b_ff1", "w_ff2", "b_ff2",
                                   "ln2_g", "ln2_b")]


class AlignerWeights(ctypes.Structure):
    """Mirror of ``ahv_aligner_weights`` (include/ahv.h)."""
    _fields_ = ([(n, _vp) for n in ("w_emb", "w_conv1", "w_conv2", "posemb", "gn_g", "gn_b")] +
                [("w_in", _vp * 2), ("b_in", _vp * 2), ("w_out", _vp * 2), ("b_out", _vp * 2),
                 ("w3d_1", _vp), ("w3d_2", _vp), ("blocks", ctypes.POINTER(BlockWeights)), ("depth", _int)])


SIGNATURES["ahv_forward_2d3d_workspace_bytes"] = (ctypes.c_size_t, [_int])
SIGNATURES["ahv_forward_2d3d_f32"] = (_int, [ctypes.POINTER(AlignerWeights), _vp, _vp, _int, _vp, ctypes.c_size_t, _vp,
                                             _vp, _vp])
SIGNATURES["ahv_score_hypotheses_backward_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64])
SIGNATURES["ahv_score_hypotheses_backward_f32"] = (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp,
                                                          ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp])
SIGNATURES["ahv_score_hypotheses_backward_saved_f32"] = SIGNATURES["ahv_score_hypotheses_backward_f32"]
SIGNATURES["ahv_score_hypotheses_train_f32"] = (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp, ctypes.c_size_t, _vp])
SIGNATURES["ahv_transformer_workspace_bytes"] = (ctypes.c_size_t, [_int])
SIGNATURES["ahv_transformer_blocks_f32"] = (_int, [ctypes.POINTER(BlockWeights), _int, _vp, _vp, _int, _vp,
                                                   ctypes.c_size_t, _vp])
SIGNATURES["ahv_topk_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64, _int])
SIGNATURES["ahv_topk_f32"] = (_int, [_vp, _int, _i64, _i64, _int, _vp, _vp, ctypes.c_size_t, _u32, _vp])
SIGNATURES["ahv_topk_merge_keys"] = (_int, [_vp, _int, _int, _int, _vp, _u32, _vp])
SIGNATURES["ahv_select_topk_f32"] = (_int, [_vp, _int, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _u32, _vp])
SIGNATURES["ahv_compose_rotations_topk_f32"] = (_int, [_vp, _int, _vp, _i64, _i64, _i64, _vp, _i64, _int, _vp, _vp])
SIGNATURES["ahv_topk_modes_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64, _int])
SIGNATURES["ahv_topk_modes_f32"] = (_int, [_vp, _vp, _i64, _int, _i64, _i64, _int, ctypes.c_float, _vp, _vp, ctypes.c_size_t, _vp])
# (scores, R, r_batch_stride, B, N, n_offset, K, min_trace, S, s_batch_stride, G, axis or NULL, axis_batch_stride, keys, workspace,
#  workspace_bytes, stream)
SIGNATURES["ahv_topk_modes_sym_f32"] = (_int, [_vp, _vp, _i64, _int, _i64, _i64, _int, ctypes.c_float, _vp, _i64, _int, _vp, _i64, _vp,
                                               _vp, ctypes.c_size_t, _vp])
# (R, r_batch_stride, B, N, S, s_batch_stride, G, axis or NULL, axis_batch_stride, anchors, K, min_trace, keep, V or NULL, R_out,
#  V_out or NULL, which, elem, trace: each or NULL, stream)
SIGNATURES["ahv_sym_fold_f32"] = (_int, [_vp, _i64, _int, _i64, _vp, _i64, _int, _vp, _i64, _vp, _int, ctypes.c_float, _i64] + [_vp] * 7)
SIGNATURES["ahv_score_rotation_grad_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64])
SIGNATURES["ahv_score_rotation_grad_f32"] = (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _int, _i64, _vp, _vp, ctypes.c_size_t,
                                                    _vp, _vp])
SIGNATURES["ahv_so3_ascent_candidates_f32"] = (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _vp])
SIGNATURES["ahv_so3_ascent_select_f32"] = (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp])
SIGNATURES["ahv_pose_posterior_state_bytes"] = (ctypes.c_size_t, [_int, _int])
SIGNATURES["ahv_pose_posterior_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64, _int])
SIGNATURES["ahv_pose_posterior_f32"] = (_int, [_vp, _vp, _i64, _int, _i64, _vp, _int, ctypes.c_float, ctypes.c_float, _vp, _vp,
                                               ctypes.c_size_t, _u32, _vp])
SIGNATURES["ahv_pose_posterior_merge"] = (_int, [_vp, _int, _int, _int, ctypes.c_float, _vp, _u32, _vp])
SIGNATURES["ahv_pose_posterior_finish_f32"] = (_int, [_vp, _int, _int, ctypes.c_float] + [_vp] * 10 + [_vp])
SIGNATURES["ahv_view_rotations_f32"] = (_int, [_vp, _i64, _vp, _int, _int, _i64, _vp, _vp])
# (scores, Q, q_batch_stride, A, weights: HOST floats, B, V, N, n_offset, min_trace, fused, best_key, flags, stream)
SIGNATURES["ahv_fuse_view_scores_f32"] = (_int, [_vp, _vp, _i64, _vp, _vp, _int, _int, _i64, _i64, ctypes.c_float, _vp, _vp, _u32,
                                                 _vp])
SIGNATURES["ahv_view_rotations_compact_workspace_bytes"] = (ctypes.c_size_t, [_int, _int, _i64])
# (Q, q_batch_stride, A, weights: HOST floats, B, V, N, min_trace, capacity, out, slot, counts, workspace, workspace_bytes, stream)
SIGNATURES["ahv_view_rotations_compact_f32"] = (_int, [_vp, _i64, _vp, _vp, _int, _int, _i64, ctypes.c_float, _i64, _vp, _vp, _vp,
                                                       _vp, ctypes.c_size_t, _vp])
# (scores, slot, weights: HOST floats, B, V, N, capacity, n_offset, fused, best_key, flags, stream)
SIGNATURES["ahv_fuse_view_scores_compact_f32"] = (_int, [_vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _vp, _vp, _u32, _vp])
# (anchor, A, B, V, K, view_idx: int32, A_sel, stream)
SIGNATURES["ahv_nearest_views_f32"] = (_int, [_vp, _vp, _int, _int, _int, _vp, _vp, _vp])
# (src, view_idx: int32 or NULL with AHV_GATHER_BROADCAST, B, V, K, L, dst, flags, stream)
SIGNATURES["ahv_gather_views_f32"] = (_int, [_vp, _vp, _int, _int, _int, _i64, _vp, _u32, _vp])
# (pair_R, pair_score, edges: int32 [E][2], B, V, E, root, A, parent_edge: int32, reached: int32, stream)
SIGNATURES["ahv_pose_graph_init_f32"] = (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _vp, _vp, _vp, _vp])
# (A, pair_R, pair_score, edges, incident: int32 [D], B, V, E, k, D, N, n_fresh, seed, counter: DEVICE int64 or NULL, sweep, sigma_rad,
#  Q, Rrel, stream)
SIGNATURES["ahv_pose_graph_propose_f32"] = (_int, [_vp] * 5 + [_int] * 5 + [_i64, _i64, ctypes.c_uint64, _vp, _int, ctypes.c_float,
                                                   _vp, _vp, _vp])
# (key, Q, B, V, k, N, A, node_score, stream)
SIGNATURES["ahv_pose_graph_commit_f32"] = (_int, [_vp, _vp, _int, _int, _int, _i64, _vp, _vp, _vp])
SIGNATURES["ahv_resample_workspace_bytes"] = (ctypes.c_size_t, [_int, _i64])
# (scores, B, N, beta, M, u: DEVICE floats or NULL, idx, workspace, workspace_bytes, flags, stream)
SIGNATURES["ahv_resample_f32"] = (_int, [_vp, _int, _i64, ctypes.c_float, _i64, _vp, _vp, _vp, ctypes.c_size_t, _u32, _vp])
SIGNATURES["ahv_compose_rotations_indexed_f32"] = (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _int, _vp, _vp])
# (idx or NULL, R, r_batch_stride, N, best_key or NULL, M, n_fresh, B, seed, step: DEVICE int64, sigma_rad, max_angle_rad, out,
#  omega or NULL, stream)
SIGNATURES["ahv_diffuse_rotations_f32"] = (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _int, ctypes.c_uint64, _vp, ctypes.c_float,
                                                  ctypes.c_float, _vp, _vp, _vp])
# (idx or NULL, R, r_batch_stride, V or NULL, v_batch_stride, N, best_key or NULL, M, n_fresh, B, seed, step: DEVICE int64,
#  sigma_rad, sigma_vel_rad, damping, max_angle_rad, max_speed_rad, coast, out, vel_out, omega or NULL, stream)
SIGNATURES["ahv_predict_rotations_f32"] = (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _int, ctypes.c_uint64, _vp]
                                           + [ctypes.c_float] * 5 + [_int, _vp, _vp, _vp, _vp])
# (R_cur, V_cur or NULL, idx, score, B, M, first, sigma0_rad, sigma_vel0_rad, n_fresh0, sigma_min_rad, sigma_max_rad, gain, rate,
#  score_floor, n_fresh_lost, control: DEVICE [B][8] words, reacquired: DEVICE bytes, stream)
SIGNATURES["ahv_track_control_f32"] = (_int, [_vp, _vp, _vp, _vp, _int, _i64, _int, ctypes.c_float, ctypes.c_float, _i64]
                                       + [ctypes.c_float] * 5 + [_i64, _vp, _vp, _vp])
# (idx or NULL, R, r_batch_stride, V or NULL, v_batch_stride, N, best_key or NULL, M, control: DEVICE [B][8] words, B, seed,
#  step: DEVICE int64, damping, max_angle_rad, max_speed_rad, coast, out, vel_out or NULL, omega or NULL, stream)
SIGNATURES["ahv_predict_rotations_ctl_f32"] = (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _int, ctypes.c_uint64, _vp]
                                               + [ctypes.c_float] * 3 + [_int, _vp, _vp, _vp, _vp])
# (seed, step: DEVICE int64, B, u: DEVICE floats, stream)
SIGNATURES["ahv_track_advance"] = (_int, [ctypes.c_uint64, _vp, _int, _vp, _vp])
# (R_cur, scores, V_cur or NULL, step: DEVICE int64, first_step, B, M, H, beta, sigma_rad, jump, damping, hist_R, hist_P or NULL,
#  hist_delta, hist_back, stream)
SIGNATURES["ahv_smooth_step_f32"] = (_int, [_vp, _vp, _vp, _vp, _i64, _int, _i64, _i64] + [ctypes.c_float] * 4 + [_vp] * 5)
# (hist_R, hist_delta, hist_back, step: DEVICE int64, first_step, B, M, H, F, path_idx, path_R, stream)
SIGNATURES["ahv_smooth_backtrace_f32"] = (_int, [_vp, _vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _vp, _vp, _vp])
# (R_cur, scores, step: DEVICE int64, first_step, B, M, H, beta, sigma_rad, jump, hist_R, hist_P or NULL, hist_alpha, hist_emit, stream)
SIGNATURES["ahv_marginal_step_f32"] = (_int, [_vp, _vp, _vp, _i64, _int, _i64, _i64] + [ctypes.c_float] * 3 + [_vp] * 5)
# (hist_R, hist_P or NULL, hist_alpha, hist_emit, step: DEVICE int64, first_step, B, M, H, F, sigma_rad, jump, logw, idx, R, stream)
SIGNATURES["ahv_marginal_smooth_f32"] = (_int, [_vp] * 5 + [_i64, _int, _i64, _i64, _i64, ctypes.c_float, ctypes.c_float] + [_vp] * 4)

# measurement / developer entry points (include/ahv_diag.h): not part of the drop-in boundary
DIAG_SIGNATURES = {
    "ahv_score_hypotheses_clocked_f32": SIGNATURES.pop("ahv_score_hypotheses_clocked_f32"),
    "ahv_diag_score_plan": (_int, [_int, _i64, _u32, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_i64)]),
}

_lib = None


class AhvError(RuntimeError):
    """A libahv_hip call returned a negative status."""


def build(force: bool = False) -> str:
    """Compile libahv_hip.so in-tree with hipcc --offload-arch=gfx950."""
    args = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    proc = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building libahv_hip.so failed:\n" + proc.stdout)
    return LIB_PATH


def load():
    """Load the library and type its entry points; raises if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime: import it FIRST so that libahv_hip.so binds to the same
    # libamdhip64 (one runtime per process: shared device context, streams and pointers).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C 3dahv_amd/csrc`."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(DIAG_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status < 0:
        msg = load().ahv_last_error().decode("utf-8", "replace")
        raise AhvError(f"{what} failed with status {status}: {msg}")
