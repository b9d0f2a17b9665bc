"""Operator mirrors of the reference's hot-path call surface, backed by libahv_hip.so.

Same names, argument meaning and error behaviour as the reference callables:

* ``rotate_volume(volume, rotation_matrix, padding_mode='zeros')``  -- utils.py:113-131
* ``forward_3d2d(img_feat, W1, W2, b2)``  -- Feature_Aligner.forward_3d2d, modules/modules.py:112-124
* ``score_features`` / ``argmax``  -- the inline lines test_co3d.py:143 / :145
* ``score_hypotheses``  -- all of the above fused into one launch (test_co3d.py:137-145)
* ``verify_pair``  -- the same with ``forward_3d2d(vol_tgt)`` (test_co3d.py:141) inside that launch
* ``rotate_volume_autograd`` / ``rotate_volume_rotation_grad``  -- ``rotate_volume`` differentiable w.r.t. the rotations too
* ``score_hypotheses_autograd`` / ``forward_3d2d_autograd`` / ``score_hypotheses_backward``  -- the same with
  autograd edges for training (infoNCE_loss, modules/model_co3d.py:41-61): HIP forward + HIP backward

Tensors must live on the GPU (``torch.device('cuda')`` is HIP on ROCm); launches go
to torch's current stream.  The plain ops carry no autograd graph; the ``*_autograd`` ones do.
"""
from __future__ import annotations

import collections
import functools
import contextvars
import math
import struct

import torch

from . import _lib

_VOL = (16, 8, 8, 8)


_SPLIT_F16 = contextvars.ContextVar("ahv_split_f16", default=False)


class split_f16_scorer:
    """``with ops.split_f16_scorer(): ...`` -- inside the block (this thread / context only) ``score_hypotheses``
    passes ``AHV_SCORE_SPLIT_F16``: both GEMMs as split-f16 MFMA products with fp32 accumulation (2.1x faster, scores as
    close to the fp64 truth as the fp32 kernel's -- DESIGN.md section 4.1).  Opt-in; the default is the all-fp32
    kernel.  The choice travels with each call as a flag bit: the library keeps no process-wide selector, so
    concurrent threads / streams cannot disturb each other.  ``score_hypotheses(..., split_f16=True)`` selects
    it for one call."""

    def __init__(self, enabled: bool = True):
        self.enabled = bool(enabled)
        self._token = None

    def __enter__(self):
        self._token = _SPLIT_F16.set(self.enabled)
        return self

    def __exit__(self, *exc):
        _SPLIT_F16.reset(self._token)
        return False


def _stream(dev=None) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _call(dev: torch.device, name: str, *args) -> None:
    """Run entry point ``name`` with ``dev`` as the current HIP device (the C side sizes its grids from
    hipGetDevice) on torch's current stream OF THAT DEVICE, so that tensors on cuda:1 are never processed on
    cuda:0's stream while cuda:0 happens to be current.  The stream is the last argument of every entry point."""
    lib = _lib.load()
    if dev.type != "cuda":
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % dev)
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def _need_gpu(*tensors: torch.Tensor) -> torch.device:
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % t.device)
        if t.device != dev:
            raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (dev, t.device))
        if t.dtype != torch.float32:
            raise RuntimeError("expected float32 tensors (the reference path is fp32), got %s" % t.dtype)
    return dev


def _refuse_grad(name: str, *tensors: torch.Tensor) -> None:
    """Ops without an autograd edge must not swallow a gradient silently."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("%s has no autograd edge: call it under torch.no_grad() / on detached tensors, or use "
                           "score_hypotheses_autograd / rotate_volume / forward_3d2d, which are differentiable" % name)


def _aligned(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """``t`` (contiguous), or a fresh copy of it when it starts off the ``nbytes`` grid: a contiguous view into the middle of
    a storage may, and the entry points refuse a misaligned pointer their kernels read through a vector type
    (include/ahv.h states which)."""
    return t if t.data_ptr() % nbytes == 0 else t.clone()


def _head(W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor):
    if W1.numel() != 32 * 384 or W2.numel() != 32 * 32 or b2.numel() != 32:
        raise RuntimeError("head weights must be (32,384[,1,1]), (32,32[,1,1]), (32,)")
    return W1.detach().reshape(32, 384).contiguous(), W2.detach().reshape(32, 32).contiguous(), b2.detach().contiguous()


def rotate_volume(volume: torch.Tensor, rotation_matrix: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    """Rotate ``volume (N,C,D,H,W)`` by ``rotation_matrix (N,3,3)``; returns a new contiguous tensor.

    The batch dimension of ``volume`` may be a stride-0 expand of one volume (what the
    reference passes): it is read once, never materialised.  Differentiable w.r.t. ``volume`` like the
    reference's (utils.py:113-131; infoNCE_loss back-propagates through it, modules/model_co3d.py:49-54): when
    autograd is recording and ``volume`` requires grad the call goes through ``_RotateVolumeFn`` (HIP forward, HIP
    adjoint).  A rotation matrix that requires grad is refused loudly by THIS function: ``rotate_volume_autograd`` is the
    form that is differentiable w.r.t. both inputs (the patched ``utils.rotate_volume`` routes such a call there), and when
    the rotated volumes only feed the reference's head and score, ``score_hypotheses`` / ``score_rotation_grad`` give
    d score / d R without materialising 32 KB per hypothesis.
    """
    if torch.is_grad_enabled():
        if rotation_matrix.requires_grad:
            raise NotImplementedError("rotate_volume: no gradient w.r.t. rotation_matrix is implemented for the op-level "
                                      "rotation (32 KB materialised per hypothesis); detach it, call "
                                      "rotate_volume_autograd (differentiable w.r.t. volume and rotation_matrix), or "
                                      "score with score_hypotheses, whose autograd edge carries d score / d R")
        if volume.requires_grad:
            return _RotateVolumeFn.apply(volume, rotation_matrix)
    return _rotate_volume_nograd(volume, rotation_matrix, padding_mode)


def rotate_volume_autograd(volume: torch.Tensor, rotation_matrix: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    """``rotate_volume`` with autograd edges to BOTH inputs, like the reference's ``F.affine_grid`` + ``F.grid_sample``
    (utils.py:113-131): the volume adjoint by ``ahv_rotate_volume_backward_f32``, the rotation gradient by
    ``ahv_rotate_volume_rotation_grad_f32`` (``rotate_volume_rotation_grad``), each only when its input needs one.  Without
    a recording graph, or with neither input requiring grad, it is the plain ``rotate_volume``."""
    if padding_mode != "zeros":
        raise NotImplementedError("only padding_mode='zeros' (the only mode the reference uses) is implemented")
    if torch.is_grad_enabled() and (volume.requires_grad or rotation_matrix.requires_grad):
        return _RotateVolumeFn.apply(volume, rotation_matrix)
    return _rotate_volume_nograd(volume, rotation_matrix, padding_mode)


def _shared_volume(volume: torch.Tensor) -> bool:
    """The stride-0 expand of one volume over the batch (what the reference passes): read once, never materialised."""
    return bool(volume.shape[0] > 1 and volume.stride(0) == 0 and volume[0].is_contiguous())


@torch.no_grad()
def rotate_volume_rotation_grad(volume: torch.Tensor, rotation_matrix: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """``d <grad_out, rotate_volume(volume, R)> / d R`` as ``(N,3,3)``: what torch autograd returns for ``rotation_matrix``
    through utils.rotate_volume (``ahv_rotate_volume_rotation_grad_f32``, include/ahv.h has the formula and the
    conventions).  ``volume (N,C,D,H,W)`` may be a stride-0 expand of one volume; ``grad_out`` is ``(N,C,D,H,W)``.  One
    workgroup per hypothesis and no atomics: a row is the same bits whatever N or the cut into calls are."""
    if volume.dim() != 5:
        raise RuntimeError("volume must be 5-D (N,C,D,H,W), got %s" % (tuple(volume.shape),))
    if rotation_matrix.dim() != 3 or tuple(rotation_matrix.shape[1:]) != (3, 3):
        raise RuntimeError("rotation_matrix must be (N,3,3), got %s" % (tuple(rotation_matrix.shape),))
    N, C, D, H, W = volume.shape
    if rotation_matrix.shape[0] != N:
        raise RuntimeError("Expected volume and rotation_matrix to have the same batch size, got %d and %d"
                           % (N, rotation_matrix.shape[0]))
    if tuple(grad_out.shape) != (N, C, D, H, W):
        raise RuntimeError("grad_out must have the rotated volumes' shape %s, got %s" % ((N, C, D, H, W), tuple(grad_out.shape)))
    dev = _need_gpu(volume, rotation_matrix, grad_out)
    volume = volume.detach()
    if _shared_volume(volume):
        src, stride = volume[0], 0
    else:
        src = volume.contiguous()
        stride = C * D * H * W
    R = rotation_matrix.detach().contiguous()
    g = grad_out.detach().contiguous()
    out = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
    _call(dev, "ahv_rotate_volume_rotation_grad_f32", g.data_ptr(), src.data_ptr(), stride, R.data_ptr(), N, C, D, H, W,
          out.data_ptr())
    return out


@torch.no_grad()
def _rotate_volume_nograd(volume: torch.Tensor, rotation_matrix: torch.Tensor, padding_mode: str = "zeros") -> torch.Tensor:
    if padding_mode != "zeros":
        raise NotImplementedError("only padding_mode='zeros' (the only mode the reference uses) is implemented")
    if volume.dim() != 5:
        raise RuntimeError("volume must be 5-D (N,C,D,H,W), got %s" % (tuple(volume.shape),))
    if rotation_matrix.dim() != 3 or tuple(rotation_matrix.shape[1:]) != (3, 3):
        raise RuntimeError("rotation_matrix must be (N,3,3), got %s" % (tuple(rotation_matrix.shape),))
    N, C, D, H, W = volume.shape
    if rotation_matrix.shape[0] != N:
        raise RuntimeError("Expected volume and rotation_matrix to have the same batch size, got %d and %d"
                           % (N, rotation_matrix.shape[0]))
    _need_gpu(volume, rotation_matrix)
    volume = volume.detach()
    if N > 1 and volume.stride(0) == 0 and volume[0].is_contiguous():
        src, stride = volume[0], 0
    else:
        src = volume.contiguous()
        stride = C * D * H * W
    R = rotation_matrix.detach().contiguous()
    out = torch.empty((N, C, D, H, W), dtype=torch.float32, device=volume.device)
    _call(out.device, "ahv_rotate_volume_f32", src.data_ptr(), stride, R.data_ptr(), N, C, D, H, W, out.data_ptr())
    return out


def forward_3d2d(img_feat: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """``(M,16,8,8,8) -> (M,32,64)``: slabs -> conv1x1 -> ReLU -> conv1x1+bias -> L2-normalise.
    When autograd is recording and an input requires grad, the call carries an autograd edge (HIP backward,
    ``_Forward3d2dFn``) -- it never silently drops a gradient."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (img_feat, W1, W2, b2)):
        return _Forward3d2dFn.apply(img_feat, W1, W2, b2)
    return _forward_3d2d_nograd(img_feat, W1, W2, b2)


@torch.no_grad()
def _forward_3d2d_nograd(img_feat: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    if img_feat.dim() != 5 or tuple(img_feat.shape[1:]) != _VOL:
        raise RuntimeError("img_feat must be (M,16,8,8,8), got %s" % (tuple(img_feat.shape),))
    _need_gpu(img_feat, W1, W2, b2)
    W1, W2, b2 = _head(W1, W2, b2)
    x = _aligned(img_feat.detach().contiguous(), 8)
    M = x.shape[0]
    out = torch.empty((M, 32, 64), dtype=torch.float32, device=x.device)
    _call(out.device, "ahv_forward_3d2d_f32", x.data_ptr(), W1.data_ptr(), W2.data_ptr(), b2.data_ptr(), M,
          out.data_ptr())
    return out


def score_features(f_src: torch.Tensor, f_tgt: torch.Tensor) -> torch.Tensor:
    """``(f_src * f_tgt[:, None]).sum(dim=2).mean(dim=-1)``: (B,N,32,64),(B,32,64) -> (B,N).  Inference only."""
    _refuse_grad("score_features", f_src, f_tgt)
    if f_src.dim() != 4 or tuple(f_src.shape[2:]) != (32, 64) or tuple(f_tgt.shape) != (f_src.shape[0], 32, 64):
        raise RuntimeError("expected f_src (B,N,32,64) and f_tgt (B,32,64)")
    _need_gpu(f_src, f_tgt)
    B, N = f_src.shape[:2]
    a, t = _aligned(f_src.detach().contiguous(), 16), _aligned(f_tgt.detach().contiguous(), 16)
    out = torch.empty((B, N), dtype=torch.float32, device=a.device)
    _call(out.device, "ahv_score_features_f32", a.data_ptr(), t.data_ptr(), B, N, out.data_ptr())
    return out


@torch.no_grad()
def unpack_best(best_key: torch.Tensor):
    """Packed keys (B,) int64 -> (best_score (B,) f32, best_idx (B,) int64)."""
    B = best_key.numel()
    score = torch.empty((B,), dtype=torch.float32, device=best_key.device)
    idx = torch.empty((B,), dtype=torch.int64, device=best_key.device)
    _call(best_key.device, "ahv_unpack_best", best_key.data_ptr(), B, score.data_ptr(), idx.data_ptr())
    return score, idx


@torch.no_grad()
def argmax(scores: torch.Tensor, n_offset: int = 0, return_key: bool = False):
    """``torch.max(scores, dim=1)`` -> (values, first maximal int64 index); (B,N) -> (B,),(B,)."""
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B,N)")
    _need_gpu(scores)
    B, N = scores.shape
    if N == 0:
        raise RuntimeError("max(): Expected reduction dim 1 to have non-zero size.")
    s = scores.detach().contiguous()
    key = torch.empty((B,), dtype=torch.int64, device=s.device)
    _call(key.device, "ahv_argmax_f32", s.data_ptr(), B, N, n_offset, key.data_ptr(), _lib.AHV_SCORE_RESET_BEST)
    if return_key:
        return key
    return unpack_best(key)


def score_hypotheses(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor,
                     W2: torch.Tensor, b2: torch.Tensor, n_offset: int = 0, want_scores: bool = True,
                     best_key: torch.Tensor | None = None, reset_best: bool | None = None,
                     split_f16: bool | None = None, clock_stamps: torch.Tensor | None = None,
                     no_teams: bool = False, spare_cus: int = 0):
    """Fused hot loop (one launch): returns ``(scores (B,N) or None, best_key (B,) int64)``.

    vol_src (B,16,8,8,8); feat_tgt (B,32,64) = forward_3d2d(vol_tgt); R (N,3,3) shared by the
    batch (modules/model.py:184) or (B,N,3,3) per sample (modules/model.py:51).  ``best_key``
    given: merge into it (chunked / multi-call N) unless ``reset_best``; else a fresh key tensor
    is reset and returned.
    Decode with ``unpack_best``; ``n_offset`` is the global index of R[0] when N is sharded.
    ``split_f16``: opt-in kernel for this call (None: the enclosing ``split_f16_scorer`` block, else fp32).
    ``clock_stamps`` (int64, 4 * CU count, zeroed): diagnostic launch that also records the shader clock.
    ``no_teams``: AHV_SCORE_NO_TEAMS -- every hypothesis by one wave.  A scheduling knob only: by default a launch's
    remainder goes to teams of four waves, whose score is the lone wave's bit for bit (a score is a function of the
    volumes, the weights and R_n alone -- not of N, of ``n_offset`` or of how a set is sharded); ``spare_cus``: compute
    units left without a workgroup of the persistent grid (a measurement knob, include/ahv_diag.h).
    With autograd recording and an input that requires grad, the returned scores carry the autograd edge of
    ``score_hypotheses_autograd`` (HIP backward) -- like the reference's op sequence, nothing is silently detached.
    """
    if (want_scores and clock_stamps is None and torch.is_grad_enabled()
            and any(t.requires_grad for t in (vol_src, feat_tgt, R, W1, W2, b2))):
        return _ScoreFn.apply(vol_src, feat_tgt, R, W1, W2, b2, n_offset, best_key, reset_best, split_f16)
    with torch.no_grad():
        return _score_hypotheses_nograd(vol_src, feat_tgt, R, W1, W2, b2, n_offset, want_scores, best_key, reset_best,
                                        split_f16, clock_stamps, no_teams=no_teams, spare_cus=spare_cus)


def score_plan(B: int, N: int, no_teams: bool = False, split_f16: bool = False, spare_cus: int = 0):
    """How a launch of B samples x N hypotheses is laid out on the current device (``ahv_diag_score_plan``, pure host
    arithmetic): ``(gx, gy, n_main)`` -- the persistent grid and how many hypotheses of each sample go to single waves; the
    rest, ``[n_main, N)``, go to teams of four.  Scores do not depend on it (a team's score is a lone wave's bit for bit)."""
    import ctypes
    flags = ((_lib.AHV_SCORE_NO_TEAMS if no_teams else 0) | (_lib.AHV_SCORE_SPLIT_F16 if split_f16 else 0) |
             (int(spare_cus) << _lib.AHV_SCORE_SPARE_CUS_SHIFT))
    gx, gy, n_main = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _lib.check(_lib.load().ahv_diag_score_plan(B, N, flags, ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(n_main)),
               "ahv_diag_score_plan")
    return gx.value, gy.value, n_main.value


def verify_pair(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                b2: torch.Tensor, n_offset: int = 0, want_scores: bool = True, best_key: torch.Tensor | None = None,
                reset_best: bool | None = None, split_f16: bool | None = None, want_feat_tgt: bool = False,
                clock_stamps: torch.Tensor | None = None, no_teams: bool = False, spare_cus: int = 0,
                scores_out: torch.Tensor | None = None):
    """The whole per-pair verify step of test_co3d.py:137-145 behind ONE entry point (``ahv_verify_pair_f32``):
    ``forward_3d2d(vol_tgt)`` is built inside the scoring launch instead of in a launch of its own.  Arguments as
    ``score_hypotheses`` with the target VOLUME ``vol_tgt (B,16,8,8,8)`` in place of ``feat_tgt``.  Returns
    ``(scores (B,N) or None, best_key (B,) int64)`` and, with ``want_feat_tgt``, the target features ``(B,32,64)`` as
    third element (always materialised for the split-f16 kernel, which runs forward_3d2d as a launch of its own).
    ``scores_out``: a contiguous float32 ``(B,N)`` tensor to write the scores to instead of a fresh one.
    Inference only (no autograd edge): with autograd recording and an input that requires grad it REFUSES (the check runs
    before the no_grad block -- as a decorator the block hid the recording state from the check, round 4) -- use
    ``forward_3d2d`` + ``score_hypotheses``, which carry the HIP backward."""
    _refuse_grad("verify_pair", vol_src, vol_tgt, R, W1, W2, b2)
    if vol_tgt.dim() != 5 or tuple(vol_tgt.shape) != tuple(vol_src.shape):
        raise RuntimeError("vol_tgt must have vol_src's shape (B,16,8,8,8), got %s" % (tuple(vol_tgt.shape),))
    split = bool(_SPLIT_F16.get() if split_f16 is None else split_f16)
    with torch.no_grad():
        feat = None
        if want_feat_tgt or split:
            feat = torch.empty((vol_src.shape[0], 32, 64), dtype=torch.float32, device=vol_src.device)
        scores, key = _score_hypotheses_nograd(vol_src, vol_tgt, R, W1, W2, b2, n_offset, want_scores, best_key, reset_best,
                                               split, clock_stamps, no_teams=no_teams, spare_cus=spare_cus,
                                               tgt_is_volume=True, feat_tgt_out=feat, scores_out=scores_out)
    return (scores, key, feat) if want_feat_tgt else (scores, key)


def _score_hypotheses_nograd(vol_src, feat_tgt, R, W1, W2, b2, n_offset, want_scores, best_key, reset_best, split_f16,
                             clock_stamps, no_teams=False, spare_cus=0, tgt_is_volume=False, feat_tgt_out=None, scores_out=None):
    if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL:
        raise RuntimeError("vol_src must be (B,16,8,8,8), got %s" % (tuple(vol_src.shape),))
    B = vol_src.shape[0]
    if not tgt_is_volume and tuple(feat_tgt.shape) != (B, 32, 64):
        raise RuntimeError("feat_tgt must be (B,32,64), got %s" % (tuple(feat_tgt.shape),))
    if R.dim() == 3 and tuple(R.shape[1:]) == (3, 3):
        N, rstride = R.shape[0], 0
    elif R.dim() == 4 and R.shape[0] == B and tuple(R.shape[2:]) == (3, 3):
        N, rstride = R.shape[1], R.shape[1] * 9
    else:
        raise RuntimeError("R must be (N,3,3) or (B,N,3,3), got %s" % (tuple(R.shape),))
    dev = _need_gpu(vol_src, feat_tgt, R, W1, W2, b2)
    W1, W2, b2 = _head(W1, W2, b2)
    vs, ft, Rc = vol_src.detach().contiguous(), feat_tgt.detach().contiguous(), R.detach().contiguous()
    if tgt_is_volume:
        ft = _aligned(ft, 8)
    scores = None
    if want_scores and scores_out is not None:
        if (scores_out.dtype != torch.float32 or tuple(scores_out.shape) != (B, N) or not scores_out.is_contiguous()
                or scores_out.device != dev):
            raise RuntimeError("scores_out must be a contiguous float32 (B,N) = %s tensor on %s" % ((B, N), dev))
        scores = scores_out
    elif want_scores:
        scores = torch.empty((B, N), dtype=torch.float32, device=dev)
    if best_key is None:
        best_key = torch.empty((B,), dtype=torch.int64, device=dev)
        reset_best = True
    elif best_key.dtype != torch.int64 or best_key.numel() != B or not best_key.is_cuda:
        raise RuntimeError("best_key must be a GPU int64 tensor of B elements")
    flags = _lib.AHV_SCORE_RESET_BEST if reset_best else 0
    if _SPLIT_F16.get() if split_f16 is None else split_f16:
        flags |= _lib.AHV_SCORE_SPLIT_F16
    if no_teams:
        flags |= _lib.AHV_SCORE_NO_TEAMS
    if not 0 <= int(spare_cus) <= 255:
        raise RuntimeError("spare_cus must be in 0..255")
    flags |= int(spare_cus) << _lib.AHV_SCORE_SPARE_CUS_SHIFT
    lib = _lib.load()
    head = (vs.data_ptr(), ft.data_ptr(), Rc.data_ptr(), rstride, n_offset, W1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
            B, N, scores.data_ptr() if scores is not None else None, best_key.data_ptr())
    if clock_stamps is not None and (clock_stamps.dtype != torch.int64 or clock_stamps.device != dev or
                                     clock_stamps.numel() < 4 * lib.ahv_device_cu_count()):
        raise RuntimeError("clock_stamps must be an int64 tensor of 4 * CU-count elements on %s" % dev)
    with torch.cuda.device(dev):
        if tgt_is_volume:
            _lib.check(lib.ahv_verify_pair_f32(*head, feat_tgt_out.data_ptr() if feat_tgt_out is not None else None, flags,
                                               clock_stamps.data_ptr() if clock_stamps is not None else None,
                                               _stream(dev)), "ahv_verify_pair_f32")
        elif clock_stamps is None:
            _lib.check(lib.ahv_score_hypotheses_f32(*head, flags, _stream(dev)), "ahv_score_hypotheses_f32")
        else:
            _lib.check(lib.ahv_score_hypotheses_clocked_f32(*head, flags, clock_stamps.data_ptr(), _stream(dev)),
                       "ahv_score_hypotheses_clocked_f32")
    return scores, best_key


@torch.no_grad()
def score_hypotheses_train(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                           b2: torch.Tensor):
    """The training forward: ``scores (B,N)`` as ``score_hypotheses`` computes them, plus the workspace in which the launch
    left every hypothesis' pre-activations (8 KB each) for ``score_hypotheses_backward(..., workspace=ws)`` -- the backward
    then skips the recompute of rotate_volume + the first projection (``ahv_score_hypotheses_train_f32``).  Returns
    ``(scores, workspace)``; the workspace serves ONE backward."""
    if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL:
        raise RuntimeError("vol_src must be (B,16,8,8,8), got %s" % (tuple(vol_src.shape),))
    B = vol_src.shape[0]
    if tuple(feat_tgt.shape) != (B, 32, 64):
        raise RuntimeError("feat_tgt must be (B,32,64), got %s" % (tuple(feat_tgt.shape),))
    N, rstride = _rot_layout(R, B)
    dev = _need_gpu(vol_src, feat_tgt, R, W1, W2, b2)
    W1c, W2c, b2c = _head(W1, W2, b2)
    vs, ft, Rc = (t.detach().contiguous() for t in (vol_src, feat_tgt, R))
    lib = _lib.load()
    nbytes = lib.ahv_score_hypotheses_backward_workspace_bytes(B, N)
    ws = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=dev)
    scores = torch.empty((B, N), dtype=torch.float32, device=dev)
    _call(dev, "ahv_score_hypotheses_train_f32", vs.data_ptr(), ft.data_ptr(), Rc.data_ptr(), rstride, W1c.data_ptr(),
          W2c.data_ptr(), b2c.data_ptr(), B, N, scores.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    return scores, ws


@torch.no_grad()
def score_hypotheses_backward(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor,
                              W2: torch.Tensor, b2: torch.Tensor, grad_scores: torch.Tensor, workspace: torch.Tensor | None = None):
    """Gradients of ``score_hypotheses`` w.r.t. ``(vol_src, feat_tgt, W1, W2, b2)`` given ``dL/dscores (B,N)``
    (three launches; what ``infoNCE_loss`` back-propagates, modules/model_co3d.py:41-61).  R's gradient is
    ``score_rotation_grad``'s.
    ``workspace``: what ``score_hypotheses_train`` returned for the SAME inputs -- the first kernel then reads the saved
    pre-activations instead of recomputing the forward (and consumes them: one backward per workspace)."""
    if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL:
        raise RuntimeError("vol_src must be (B,16,8,8,8), got %s" % (tuple(vol_src.shape),))
    B = vol_src.shape[0]
    if tuple(feat_tgt.shape) != (B, 32, 64):
        raise RuntimeError("feat_tgt must be (B,32,64), got %s" % (tuple(feat_tgt.shape),))
    N, rstride = _rot_layout(R, B)
    if tuple(grad_scores.shape) != (B, N):
        raise RuntimeError("grad_scores must be (B,N) = %s, got %s" % ((B, N), tuple(grad_scores.shape)))
    dev = _need_gpu(vol_src, feat_tgt, R, W1, W2, b2, grad_scores)
    W1c, W2c, b2c = _head(W1, W2, b2)
    vs, ft, Rc, gs = (t.detach().contiguous() for t in (vol_src, feat_tgt, R, grad_scores))
    lib = _lib.load()
    nbytes = lib.ahv_score_hypotheses_backward_workspace_bytes(B, N)
    saved = workspace is not None
    if saved:
        if workspace.device != dev or workspace.dtype != torch.float32 or workspace.numel() * 4 < nbytes:
            raise RuntimeError("workspace is not the one score_hypotheses_train returned for these shapes")
        ws = workspace
    else:
        ws = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=dev)
    g_vol = torch.empty((B,) + _VOL, dtype=torch.float32, device=dev)
    g_ft = torch.empty((B, 32, 64), dtype=torch.float32, device=dev)
    g_W1 = torch.empty((32, 384), dtype=torch.float32, device=dev)
    g_W2 = torch.empty((32, 32), dtype=torch.float32, device=dev)
    g_b2 = torch.empty((32,), dtype=torch.float32, device=dev)
    _call(dev, "ahv_score_hypotheses_backward_saved_f32" if saved else "ahv_score_hypotheses_backward_f32", vs.data_ptr(),
          ft.data_ptr(), Rc.data_ptr(), rstride,
          W1c.data_ptr(), W2c.data_ptr(), b2c.data_ptr(), B, N, gs.data_ptr(), ws.data_ptr(), ws.numel() * 4,
          g_vol.data_ptr(), g_ft.data_ptr(), g_W1.data_ptr(), g_W2.data_ptr(), g_b2.data_ptr())
    return g_vol, g_ft, g_W1, g_W2, g_b2


class _RotateVolumeFn(torch.autograd.Function):
    """Differentiable ``rotate_volume``: HIP gather forward, HIP scatter adjoint for the volume, HIP gather for the
    rotations (``rotate_volume_rotation_grad``).  A stride-0 batch (``v[None].expand(N, ...)``) is read once in the
    forward; its gradient is accumulated into ONE volume on the device.  Autograd's expand-backward then sums the N rows of
    what this function returns, so row 0 carries that volume and the other rows are zero (exact; no division by N).
    The volume is saved only when the rotations need a gradient (a shared one as its 32 KB base)."""

    @staticmethod
    def forward(ctx, volume, rotation_matrix):
        out = _rotate_volume_nograd(volume, rotation_matrix)
        ctx.shared = _shared_volume(volume)
        ctx.vshape = tuple(volume.shape)
        if ctx.needs_input_grad[1]:
            v = volume.detach()
            ctx.save_for_backward(rotation_matrix.detach().contiguous(), v[0] if ctx.shared else v.contiguous())
        else:
            ctx.save_for_backward(rotation_matrix.detach().contiguous())
        return out

    @staticmethod
    def backward(ctx, grad_out):
        R = ctx.saved_tensors[0]
        N, C, D, H, W = ctx.vshape
        g = grad_out.contiguous()
        dev = g.device
        g_R = None
        if ctx.needs_input_grad[1]:
            vol = ctx.saved_tensors[1]
            g_R = rotate_volume_rotation_grad(vol[None].expand(N, -1, -1, -1, -1) if ctx.shared else vol, R, g)
        if not ctx.needs_input_grad[0]:
            return None, g_R
        if ctx.shared:
            gv = torch.empty((1, C, D, H, W), dtype=torch.float32, device=dev)
            _call(dev, "ahv_rotate_volume_backward_f32", g.data_ptr(), 0, R.data_ptr(), N, C, D, H, W, gv.data_ptr())
            # the expand's backward sums over the batch: put the whole sum in row 0
            full = torch.zeros((N, C, D, H, W), dtype=torch.float32, device=dev)
            full[0] = gv[0]
            return full, g_R
        gv = torch.empty((N, C, D, H, W), dtype=torch.float32, device=dev)
        _call(dev, "ahv_rotate_volume_backward_f32", g.data_ptr(), C * D * H * W, R.data_ptr(), N, C, D, H, W,
              gv.data_ptr())
        return gv, g_R


class _ScoreFn(torch.autograd.Function):
    """Differentiable fused scorer: forward = one fused launch, backward = ``score_hypotheses_backward`` for the volume, the
    target features and the head weights and ``score_rotation_grad`` for R (a shared (N,3,3) set receives the sum over the
    batch).  Each runs only when one of its inputs needs a gradient."""

    @staticmethod
    def forward(ctx, vol_src, feat_tgt, R, W1, W2, b2, n_offset=0, best_key=None, reset_best=None, split_f16=None, need_key=True):
        ctx.ws = None
        plain = n_offset == 0 and best_key is None and not split_f16 and (split_f16 is not None or not _SPLIT_F16.get())
        # the saved pre-activations serve the volume / feature / weight gradients; R's gradient brings its own workspace
        plain = plain and any(ctx.needs_input_grad[i] for i in (0, 1, 3, 4, 5))
        if plain:
            # the training forward: the same scores, and the pre-activations kept for the backward (no recompute there);
            # the arg-max key of the inference launch is not produced -- callers of the differentiable form use the scores
            scores, ctx.ws = score_hypotheses_train(vol_src, feat_tgt, R, W1, W2, b2)
            if need_key:   # (score_hypotheses' contract: the packed arg-max key beside the scores)
                key = argmax(scores, return_key=True)
            else:
                key = torch.full((vol_src.shape[0],), _lib.AHV_KEY_EMPTY, dtype=torch.int64, device=scores.device)
        else:
            scores, key = _score_hypotheses_nograd(vol_src, feat_tgt, R, W1, W2, b2, n_offset, True, best_key, reset_best,
                                                   split_f16, None)
        ctx.save_for_backward(vol_src, feat_tgt, R, W1, W2, b2)
        ctx.mark_non_differentiable(key)
        return scores, key

    @staticmethod
    def backward(ctx, grad_scores, _grad_key):
        vol_src, feat_tgt, R, W1, W2, b2 = ctx.saved_tensors
        ws, ctx.ws = ctx.ws, None   # one backward per workspace: a second one (retain_graph) recomputes the forward
        gs = grad_scores.contiguous()
        need = ctx.needs_input_grad
        g_R = None
        if need[2]:   # before the other backward: that one consumes the saved workspace, this one brings its own
            g_R = score_rotation_grad(vol_src, feat_tgt, R, W1, W2, b2, gs)
            if R.dim() == 3:
                g_R = g_R.sum(dim=0)
        if not (need[0] or need[1] or need[3] or need[4] or need[5]):
            return (None, None, g_R) + (None,) * 8
        g_vol, g_ft, g_W1, g_W2, g_b2 = score_hypotheses_backward(vol_src, feat_tgt, R, W1, W2, b2, gs, workspace=ws)
        return (g_vol, g_ft, g_R, g_W1.reshape(W1.shape), g_W2.reshape(W2.shape), g_b2.reshape(b2.shape),
                None, None, None, None, None)


def score_hypotheses_autograd(vol_src, feat_tgt, R, W1, W2, b2) -> torch.Tensor:
    """``scores (B,N)`` with autograd support for vol_src, feat_tgt, the head weights (training path) and R."""
    return _ScoreFn.apply(vol_src, feat_tgt, R, W1, W2, b2, 0, None, None, None, False)[0]


class _Forward3d2dFn(torch.autograd.Function):
    """Differentiable ``forward_3d2d``.  The backward reuses the scorer's: with R = identity the scorer's feature
    IS forward_3d2d(vol) (an identity rotation reproduces the voxels exactly), and for L = sum(dF * f) the
    gradients equal those of 64 * score computed against "target" dF -- so one call with N = 1, R = I,
    feat_tgt = dF and grad_scores = 64 returns d vol, d W1, d W2, d b2."""

    @staticmethod
    def forward(ctx, vol, W1, W2, b2):
        ctx.save_for_backward(vol, W1, W2, b2)
        return _forward_3d2d_nograd(vol, W1, W2, b2)

    @staticmethod
    def backward(ctx, dF):
        vol, W1, W2, b2 = ctx.saved_tensors
        M = vol.shape[0]
        eye = torch.eye(3, dtype=torch.float32, device=vol.device).reshape(1, 3, 3)
        gs = torch.full((M, 1), 64.0, dtype=torch.float32, device=vol.device)
        g_vol, _, g_W1, g_W2, g_b2 = score_hypotheses_backward(vol, dF.contiguous(), eye, W1, W2, b2, gs)
        return g_vol, g_W1.reshape(W1.shape), g_W2.reshape(W2.shape), g_b2.reshape(b2.shape)


def forward_3d2d_autograd(img_feat, W1, W2, b2) -> torch.Tensor:
    """``forward_3d2d`` with autograd support for the volume and the head weights (training path)."""
    return _Forward3d2dFn.apply(img_feat, W1, W2, b2)


def _rot_layout(R: torch.Tensor, B: int):
    if R.dim() == 3 and tuple(R.shape[1:]) == (3, 3):
        return R.shape[0], 0
    if R.dim() == 4 and R.shape[0] == B and tuple(R.shape[2:]) == (3, 3):
        return R.shape[1], R.shape[1] * 9
    raise RuntimeError("R must be (N,3,3) or (B,N,3,3), got %s" % (tuple(R.shape),))


@torch.no_grad()
def reset_best(best_key: torch.Tensor) -> torch.Tensor:
    """``best_key[:] = AHV_KEY_EMPTY`` (one tiny launch): a key tensor ready to be merged into."""
    if best_key.dtype != torch.int64 or not best_key.is_cuda:
        raise RuntimeError("best_key must be a GPU int64 tensor")
    _call(best_key.device, "ahv_reset_best", best_key.data_ptr(), best_key.numel())
    return best_key


@torch.no_grad()
def select_rotation(best_key: torch.Tensor, R: torch.Tensor, n_offset: int = 0, reset_key: bool = False, out=None):
    """(best_score (B,), best_idx (B,) global int64, R_pred (B,3,3)) in ONE launch:
    ``pred_sim, pred_index = torch.max(...)``; ``proposals[pred_index]`` (test_co3d.py:145-146).
    ``reset_key``: hand ``best_key`` back EMPTY (AHV_SELECT_RESET_KEY), ready for the next step's scorer.
    ``out``: ``(score, idx, R_pred)`` tensors of those shapes to write to (then nothing is allocated)."""
    B = best_key.numel()
    _need_gpu(R)
    N, rstride = _rot_layout(R, B)
    Rc = R.detach().contiguous()
    dev = Rc.device
    if out is not None:
        score, idx, R_out = out
        for t, dt, shape in ((score, torch.float32, (B,)), (idx, torch.int64, (B,)), (R_out, torch.float32, (B, 3, 3))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise RuntimeError("out must be (score (B,) float32, idx (B,) int64, R_pred (B,3,3) float32), contiguous, on %s" % dev)
    else:
        score = torch.empty((B,), dtype=torch.float32, device=dev)
        idx = torch.empty((B,), dtype=torch.int64, device=dev)
        R_out = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    _call(dev, "ahv_select_rotation_f32", best_key.data_ptr(), Rc.data_ptr(), rstride, n_offset, N, B,
          R_out.data_ptr(), score.data_ptr(), idx.data_ptr(), _lib.AHV_SELECT_RESET_KEY if reset_key else 0)
    return score, idx, R_out


@torch.no_grad()
def compose_rotations(best_key: torch.Tensor, R: torch.Tensor, D: torch.Tensor, n_offset: int = 0,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """Refinement hypotheses ``out[b, n] = R[idx_b] @ D[n]`` with idx_b decoded from the packed key on the
    device (coarse-to-fine, BASELINE.json configs[4]).  R (N,3,3) or (B,N,3,3); D (N2,3,3) -> (B,N2,3,3)."""
    B = best_key.numel()
    _need_gpu(R, D)
    N, rstride = _rot_layout(R, B)
    if D.dim() != 3 or tuple(D.shape[1:]) != (3, 3):
        raise RuntimeError("D must be (N2,3,3)")
    N2 = D.shape[0]
    Rc, Dc = R.detach().contiguous(), D.detach().contiguous()
    if out is None:
        out = torch.empty((B, N2, 3, 3), dtype=torch.float32, device=Rc.device)
    _call(out.device, "ahv_compose_rotations_f32", best_key.data_ptr(), Rc.data_ptr(), rstride, n_offset, N,
          Dc.data_ptr(), N2, B, out.data_ptr())
    return out


# ---- K best hypotheses -------------------------------------------------------------------------------
# A list is (B, K) int64 packed keys in descending order, distinct, padded with AHV_KEY_EMPTY: the first K entries of
# torch.sort(scores, dim=1, descending=True, stable=True) -- NOT torch.topk's order, which leaves ties unspecified.

# (device, B, N, K) -> workspace: static buffers, so that a captured graph replays on the same memory.  One buffer per shape,
# shared by every caller: calls of one shape on DIFFERENT streams at the same time would race on it between the two launches
# (issue them on one stream), and a buffer stays for every distinct N that was ever used (8 * min(N/1024, 63) * B * K bytes).
_TOPK_WS = {}


def _workspace(cache: dict, key: tuple, nbytes: int, dtype: torch.dtype, given: torch.Tensor | None = None):
    """``(workspace or None, bytes it holds)`` for a call that needs ``nbytes``: the caller's tensor when ``given``, else the
    static buffer ``cache[key]`` (``key[0]`` is the device), allocated on first use; none at all when nothing is needed.  With
    ``given`` nothing is allocated (capture)."""
    dev = key[0]
    ws = given
    if ws is None and nbytes:
        ws = cache.get(key)
        if ws is None:
            ws = cache[key] = torch.empty((nbytes // dtype.itemsize,), dtype=dtype, device=dev)
    have = 0
    if ws is not None:
        if ws.device != dev or not ws.is_contiguous():
            raise RuntimeError("workspace must be a contiguous tensor on %s" % dev)
        have = ws.numel() * ws.element_size()
    return ws, have


def _topk_k(k) -> int:
    k = int(k)
    if not 1 <= k <= _lib.AHV_TOPK_MAX_K:
        raise RuntimeError("K = %d outside 1..%d" % (k, _lib.AHV_TOPK_MAX_K))
    return k


def _topk_list(keys: torch.Tensor, what: str = "keys"):
    if keys.dim() != 2 or keys.dtype != torch.int64:
        raise RuntimeError("%s must be a (B,K) int64 tensor" % what)
    if not keys.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % keys.device)
    if not keys.is_contiguous():
        raise RuntimeError("%s must be contiguous" % what)
    return keys.shape[0], _topk_k(keys.shape[1])


@torch.no_grad()
def topk(scores: torch.Tensor, k: int, n_offset: int = 0, keys: torch.Tensor | None = None, reset: bool | None = None):
    """The K best of ``scores (B,N)`` as packed keys ``(B,K)`` (``ahv_topk_f32``).  ``keys`` given: merge into that list
    (chunked N, shards with their ``n_offset``) unless ``reset``; else a fresh list is returned.  ``keys[:, 0]`` is the
    arg-max key.  Decode with ``select_topk``."""
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B,N)")
    k = _topk_k(k)
    dev = _need_gpu(scores)
    B, N = scores.shape
    if keys is None:
        keys = torch.empty((B, k), dtype=torch.int64, device=dev)
        reset = True
    elif _topk_list(keys) != (B, k) or keys.device != dev:
        raise RuntimeError("keys must be a (B,K) = %s int64 tensor on %s" % ((B, k), dev))
    s = scores.detach().contiguous()
    ws, have = _workspace(_TOPK_WS, (dev, B, N, k), _lib.load().ahv_topk_workspace_bytes(B, N, k), torch.int64)
    _call(dev, "ahv_topk_f32", s.data_ptr(), B, N, n_offset, k, keys.data_ptr(), ws.data_ptr() if ws is not None else None,
          have, _lib.AHV_TOPK_RESET_LIST if reset else 0)
    return keys


@torch.no_grad()
def merge_topk(lists: torch.Tensor, keys: torch.Tensor | None = None, reset: bool | None = None):
    """``lists (P,B,K)`` -> one list ``(B,K)`` (``ahv_topk_merge_keys``): what follows an all-gather of per-rank lists.
    Duplicate keys are kept once, so a list merged twice changes nothing.  ``keys`` given: merge into it unless ``reset``."""
    if lists.dim() != 3 or lists.dtype != torch.int64:
        raise RuntimeError("lists must be a (P,B,K) int64 tensor")
    if not lists.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % lists.device)
    P, B, k = lists.shape
    k = _topk_k(k)
    if keys is None:
        keys = torch.empty((B, k), dtype=torch.int64, device=lists.device)
        reset = True
    elif _topk_list(keys) != (B, k) or keys.device != lists.device:
        raise RuntimeError("keys must be a (B,K) = %s int64 tensor on %s" % ((B, k), lists.device))
    ls = lists.contiguous()
    _call(ls.device, "ahv_topk_merge_keys", ls.data_ptr(), P, B, k, keys.data_ptr(), _lib.AHV_TOPK_RESET_LIST if reset else 0)
    return keys


@torch.no_grad()
def select_topk(keys: torch.Tensor, R: torch.Tensor, n_offset: int = 0, reset_keys: bool = False):
    """``(scores (B,K), idx (B,K) global int64, R (B,K,3,3))`` of a list in ONE launch (``ahv_select_topk_f32``); an empty
    slot gives -inf, -1 and a zero row; so does (for the row) a slot owned by another shard.  ``reset_keys``: hand the
    list back empty."""
    B, k = _topk_list(keys)
    _need_gpu(R)
    if R.device != keys.device:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (keys.device, R.device))
    N, rstride = _rot_layout(R, B)
    Rc = R.detach().contiguous()
    dev = Rc.device
    score = torch.empty((B, k), dtype=torch.float32, device=dev)
    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    R_out = torch.empty((B, k, 3, 3), dtype=torch.float32, device=dev)
    _call(dev, "ahv_select_topk_f32", keys.data_ptr(), k, Rc.data_ptr(), rstride, n_offset, N, B, R_out.data_ptr(),
          score.data_ptr(), idx.data_ptr(), _lib.AHV_SELECT_RESET_KEY if reset_keys else 0)
    return score, idx, R_out


@torch.no_grad()
def compose_rotations_topk(keys: torch.Tensor, R: torch.Tensor, D: torch.Tensor, n_offset: int = 0,
                           out: torch.Tensor | None = None) -> torch.Tensor:
    """Refinement hypotheses around K seeds: ``out[b, k * N2 + n] = R[idx_{b,k}] @ D[n]`` -> (B, K*N2, 3, 3)
    (``ahv_compose_rotations_topk_f32``); at K = 1 it is ``compose_rotations`` bit for bit."""
    B, k = _topk_list(keys)
    _need_gpu(R, D)
    if R.device != keys.device:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (keys.device, R.device))
    N, rstride = _rot_layout(R, B)
    if D.dim() != 3 or tuple(D.shape[1:]) != (3, 3):
        raise RuntimeError("D must be (N2,3,3)")
    N2 = D.shape[0]
    Rc, Dc = R.detach().contiguous(), D.detach().contiguous()
    if out is None:
        out = torch.empty((B, k * N2, 3, 3), dtype=torch.float32, device=Rc.device)
    elif tuple(out.shape) != (B, k * N2, 3, 3) or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous (B, K*N2, 3, 3) tensor")
    _call(out.device, "ahv_compose_rotations_topk_f32", keys.data_ptr(), k, Rc.data_ptr(), rstride, n_offset, N,
          Dc.data_ptr(), N2, B, out.data_ptr())
    return out


def score_hypotheses_topk(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                          b2: torch.Tensor, k: int, n_offset: int = 0, keys: torch.Tensor | None = None,
                          reset: bool | None = None, **kw):
    """``score_hypotheses`` with the scores kept, followed by ``topk`` on them: returns
    ``(scores (B,N), best_key (B,), keys (B,K))``; ``best_key`` is the fused launch's arg-max key and equals ``keys[:, 0]``
    for a fresh list.  ``keys`` / ``reset`` as in ``topk``; other keywords go to ``score_hypotheses``."""
    k = _topk_k(k)
    scores, best_key = score_hypotheses(vol_src, feat_tgt, R, W1, W2, b2, n_offset=n_offset, want_scores=True, **kw)
    return scores, best_key, topk(scores, k, n_offset=n_offset, keys=keys, reset=reset)


def verify_pair_topk(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                     b2: torch.Tensor, k: int, n_offset: int = 0, keys: torch.Tensor | None = None,
                     reset: bool | None = None, want_feat_tgt: bool = False, **kw):
    """``verify_pair`` with the scores kept, followed by ``topk`` on them: returns ``(scores (B,N), best_key (B,),
    keys (B,K))`` and, with ``want_feat_tgt``, the target features as fourth element."""
    k = _topk_k(k)
    r = verify_pair(vol_src, vol_tgt, R, W1, W2, b2, n_offset=n_offset, want_scores=True, want_feat_tgt=want_feat_tgt, **kw)
    out = (r[0], r[1], topk(r[0], k, n_offset=n_offset, keys=keys, reset=reset))
    return out + (r[2],) if want_feat_tgt else out


# ---- distinct pose modes --------------------------------------------------------------------------------------
# (device, B, N) -> alive-state workspace of topk_modes: static like _TOPK_WS, and under the same rule (one stream per shape)
_MODES_WS = {}


def min_trace(min_angle_deg) -> float:
    """``tau = 1 + 2 cos(theta)`` in double precision, rounded to fp32: what ``ahv_topk_modes_f32`` takes as ``min_trace``."""
    theta = float(min_angle_deg)
    if not 0.0 < theta < 180.0:
        raise RuntimeError("min_angle_deg = %r outside (0, 180)" % (min_angle_deg,))
    tau = float(torch.tensor(1.0 + 2.0 * math.cos(math.radians(theta)), dtype=torch.float64).to(torch.float32))
    if not -1.0 < tau < 3.0:
        raise RuntimeError("min_angle_deg = %r: 1 + 2 cos(theta) rounds to %r in fp32, outside (-1, 3)" % (min_angle_deg, tau))
    return tau


def topk_modes_workspace(B: int, N: int, k: int, device) -> torch.Tensor | None:
    """A workspace for ``topk_modes`` on (B, N, k): allocate it once, pass it to every call (no allocation under capture)."""
    nbytes = _lib.load().ahv_topk_modes_workspace_bytes(B, N, _topk_k(k))
    return torch.empty((nbytes // 8,), dtype=torch.int64, device=device) if nbytes else None


@torch.no_grad()
def topk_modes(scores: torch.Tensor, R: torch.Tensor, k: int, min_angle_deg: float, n_offset: int = 0,
               keys: torch.Tensor | None = None, workspace: torch.Tensor | None = None, symmetry=None):
    """Up to K distinct pose modes of ``scores (B,N)`` over the hypotheses ``R (N,3,3)`` / ``(B,N,3,3)`` as packed keys
    ``(B,K)`` (``ahv_topk_modes_f32``): the K-best order with every hypothesis within ``min_angle_deg`` of an earlier entry
    left out, padded with AHV_KEY_EMPTY when the set holds fewer modes.  ``keys`` is OVERWRITTEN (modes do not merge: select
    once over the whole set -- ``dist.all_gather_scores`` for shards); ``workspace``: an int64 tensor of
    ``ahv_topk_modes_workspace_bytes`` bytes (``topk_modes_workspace``), else a static one per shape.  With both given the call
    allocates nothing.  Decode with ``select_topk``.  ``symmetry`` (a ``rotations.Symmetry`` in the source view's frame): modes are
    distinct MODULO the group (``ahv_topk_modes_sym_f32``) -- a hypothesis dies when any pose equivalent to it is within
    ``min_angle_deg`` of the winner; same list format, same workspace."""
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B,N)")
    k = _topk_k(k)
    tau = min_trace(min_angle_deg)
    if symmetry is not None and not hasattr(symmetry, "S"):
        raise RuntimeError("symmetry must be a rotations.Symmetry, got %r" % (type(symmetry).__name__,))
    dev = _need_gpu(scores, R)
    sym = _sym_args(symmetry, scores.shape[0], dev) if symmetry is not None else None
    B, N = scores.shape
    n_rot, rstride = _rot_layout(R, B)
    if n_rot != N:
        raise RuntimeError("R holds %d hypotheses, scores %d" % (n_rot, N))
    if keys is None:
        keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    elif _topk_list(keys) != (B, k) or keys.device != dev:
        raise RuntimeError("keys must be a (B,K) = %s int64 tensor on %s" % ((B, k), dev))
    s, Rc = scores.detach().contiguous(), R.detach().contiguous()
    workspace, have = _workspace(_MODES_WS, (dev, B, N), _lib.load().ahv_topk_modes_workspace_bytes(B, N, k), torch.int64,
                                 workspace)
    if sym is not None:
        _call(dev, "ahv_topk_modes_sym_f32", s.data_ptr(), Rc.data_ptr(), rstride, B, N, n_offset, k, tau, *_sym_ptrs(sym),
              keys.data_ptr(), workspace.data_ptr() if workspace is not None else None, have)
        return keys
    _call(dev, "ahv_topk_modes_f32", s.data_ptr(), Rc.data_ptr(), rstride, B, N, n_offset, k, tau, keys.data_ptr(),
          workspace.data_ptr() if workspace is not None else None, have)
    return keys


def verify_pair_modes(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                      b2: torch.Tensor, k: int, min_angle_deg: float, keys: torch.Tensor | None = None,
                      workspace: torch.Tensor | None = None, symmetry=None, **kw):
    """The verify step with distinct modes: ``verify_pair`` with the scores kept -> ``topk_modes`` -> ``select_topk``.
    Returns ``(mode_scores (B,K), mode_idx (B,K), R_modes (B,K,3,3))``; a slot past the last mode holds -inf, -1 and a zero
    matrix.  ``symmetry``: as in ``topk_modes``.  Other keywords go to ``verify_pair``."""
    k = _topk_k(k)
    scores = verify_pair(vol_src, vol_tgt, R, W1, W2, b2, want_scores=True, **kw)[0]
    return select_topk(topk_modes(scores, R, k, min_angle_deg, keys=keys, workspace=workspace, symmetry=symmetry), R)


# ---- pose selection modulo a symmetry group --------------------------------------------------------------------
# A ``rotations.Symmetry`` in the SOURCE VIEW'S frame makes R and R S the same pose (include/ahv.h, "Pose selection modulo an
# object's symmetry group").  ``topk_modes(symmetry=)`` selects modes of the quotient; ``sym_fold`` moves every hypothesis to the
# member of its orbit nearest an anchor, after which the plain posterior, tracker and smoothers see one fundamental domain.

SymFold = collections.namedtuple("SymFold", ["R", "which", "elem", "trace", "V"])


def _sym_args(symmetry, B: int, dev):
    """``(S, s_batch_stride, G, axis or None, axis_batch_stride)`` of a ``rotations.Symmetry`` for B samples on ``dev``."""
    S, axis = getattr(symmetry, "S", None), getattr(symmetry, "axis", None)
    if S is None:
        raise RuntimeError("symmetry must be a rotations.Symmetry, got %r" % (type(symmetry).__name__,))
    _need_gpu(*((S,) if axis is None else (S, axis)))
    if S.device != dev:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (dev, S.device))
    G = S.shape[-3]
    if not 1 <= G <= _lib.AHV_SYM_MAX_ELEMENTS:
        raise RuntimeError("G = %d outside 1..%d" % (G, _lib.AHV_SYM_MAX_ELEMENTS))
    if S.dim() == 4 and S.shape[0] != B:
        raise RuntimeError("symmetry holds %d samples, the call %d" % (S.shape[0], B))
    if axis is not None and axis.dim() == 2 and axis.shape[0] != B:
        raise RuntimeError("symmetry axis holds %d samples, the call %d" % (axis.shape[0], B))
    S = S.contiguous()
    axis = None if axis is None else axis.contiguous()
    return S, (G * 9 if S.dim() == 4 else 0), G, axis, (3 if axis is not None and axis.dim() == 2 else 0)


def _sym_ptrs(sym):
    S, sstride, G, axis, astride = sym
    return S.data_ptr(), sstride, G, (axis.data_ptr() if axis is not None else None), astride


@torch.no_grad()
def sym_fold(R: torch.Tensor, symmetry, anchors: torch.Tensor, min_angle_deg: float | None = None, keep: int = 0,
             V: torch.Tensor | None = None, out: torch.Tensor | None = None, V_out: torch.Tensor | None = None,
             want_info: bool = True) -> SymFold:
    """Fold the hypotheses ``R (N,3,3)`` / ``(B,N,3,3)`` into the fundamental domain around ``anchors (B,K,3,3)`` (K <= 16; an
    all-zero anchor is an empty slot) modulo ``symmetry`` (``ahv_sym_fold_f32``, one launch): hypothesis n takes the FIRST anchor k
    with an equivalent pose within ``min_angle_deg`` (``None``: no limit, so the first non-empty anchor) and becomes that pose,
    ``R_n S_g* Rot(axis, phi*)``; a body-frame velocity ``V (B,N,3)`` follows as ``(S_g* Rot)^T v``.  Returns ``SymFold(R (B,N,3,3),
    which (B,N) int32, elem (B,N) int32, trace (B,N), V)``: the anchor, the group element and the symmetric trace t_G, -1 / -1 / NaN
    for a hypothesis no anchor took (copied byte for byte) and for the slots ``n < keep`` (always copied).  ``out`` / ``V_out``:
    where to write -- ``out`` may be ``R`` itself when R is per-sample and ``V_out`` may be ``V`` (in place); the anchors must not
    overlap ``out``.  ``want_info=False``: ``which``, ``elem`` and ``trace`` are not written (``None``); with ``out`` (and
    ``V_out``) the call then allocates nothing."""
    if anchors.dim() != 4 or tuple(anchors.shape[2:]) != (3, 3):
        raise RuntimeError("anchors must be (B,K,3,3), got %s" % (tuple(anchors.shape),))
    B, K = anchors.shape[:2]
    if not 1 <= K <= _lib.AHV_SYM_FOLD_MAX_ANCHORS:
        raise RuntimeError("K = %d outside 1..%d" % (K, _lib.AHV_SYM_FOLD_MAX_ANCHORS))
    tau = -math.inf if min_angle_deg is None else min_trace(min_angle_deg)
    N, rstride = _rot_layout(R, B)
    keep = int(keep)
    if not 0 <= keep <= N:
        raise RuntimeError("keep = %d outside 0..N = %d" % (keep, N))
    dev = _need_gpu(*((R, anchors) if V is None else (R, anchors, V)))
    sym = _sym_args(symmetry, B, dev)
    if V is not None and (tuple(V.shape) != (B, N, 3) or not V.is_contiguous()):
        raise RuntimeError("V must be a contiguous (B,N,3) tensor")
    if V is None and V_out is not None:
        raise RuntimeError("V_out without V")
    if R.data_ptr() == (out.data_ptr() if out is not None else 0) and (rstride == 0 and B > 1 or not R.is_contiguous()):
        raise RuntimeError("in place needs a contiguous per-sample R")
    Rc, Ac = R.detach().contiguous(), anchors.detach().contiguous()
    if out is None:
        out = torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, N, 3, 3) or not out.is_contiguous() or out.device != dev or out.dtype != torch.float32:
        raise RuntimeError("out must be a contiguous float32 (B,N,3,3) = %s tensor on %s" % ((B, N, 3, 3), dev))
    if V is not None:
        if V_out is None:
            V_out = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        elif tuple(V_out.shape) != (B, N, 3) or not V_out.is_contiguous() or V_out.device != dev or V_out.dtype != torch.float32:
            raise RuntimeError("V_out must be a contiguous float32 (B,N,3) tensor on %s" % (dev,))
    which = elem = trace = None
    if want_info:
        which = torch.empty((B, N), dtype=torch.int32, device=dev)
        elem = torch.empty((B, N), dtype=torch.int32, device=dev)
        trace = torch.empty((B, N), dtype=torch.float32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _call(dev, "ahv_sym_fold_f32", Rc.data_ptr(), rstride, B, N, *_sym_ptrs(sym), Ac.data_ptr(), K, tau, keep, ptr(V), out.data_ptr(),
          ptr(V_out), ptr(which), ptr(elem), ptr(trace))
    return SymFold(out, which, elem, trace, V_out)


# ---- pose posterior --------------------------------------------------------------------------------------------
# The softmax of the scores at temperature T as a distribution over the hypotheses (``ahv_pose_posterior_f32``, include/ahv.h):
# its log-partition, entropy and mean score, the mass inside a geodesic cap around each of K anchors (first match) and in the
# rest, and the mean pose and angular spread of every bucket and of the whole set.  A STATE is a ``(B, stride)`` uint8 tensor
# (``ahv_pose_posterior_state_bytes``): calls merge into it, states of shards merge (``merge_posterior``), and
# ``pose_posterior_finish`` turns one into numbers.

# (device, B, N, K) -> workspace (the partial states of one call): static like _TOPK_WS, and under the same rule
_POSTERIOR_WS = {}

PosePosterior = collections.namedtuple(
    "PosePosterior", ["log_z", "entropy", "mean_score", "n_excluded", "mode_prob", "rest_prob", "mode_R_mean", "R_mean",
                      "mode_spread_deg", "spread_deg", "state"])


def inverse_temperature(temperature) -> float:
    """``beta = 1 / T`` in double precision, rounded to fp32: what the posterior entry points take as ``beta``."""
    T = float(temperature)
    if not (T > 0.0 and math.isfinite(T)):
        raise RuntimeError("temperature = %r must be finite and > 0" % (temperature,))
    beta = float(torch.tensor(1.0 / T, dtype=torch.float64).to(torch.float32))
    if not (beta > 0.0 and math.isfinite(beta)):
        raise RuntimeError("temperature = %r: 1 / T rounds to %r in fp32, it must be finite and > 0" % (temperature, beta))
    return beta


def _posterior_k(k) -> int:
    k = int(k)
    if not 0 <= k <= _lib.AHV_POSTERIOR_MAX_MODES:
        raise RuntimeError("K = %d outside 0..%d" % (k, _lib.AHV_POSTERIOR_MAX_MODES))
    return k


def _posterior_state(state: torch.Tensor, k: int, what: str = "state"):
    """(B, stride) of a state tensor ``(..., B, stride)`` uint8 for K = k."""
    stride = _lib.load().ahv_pose_posterior_state_bytes(1, k)
    if state.dtype != torch.uint8 or state.dim() < 2 or state.shape[-1] != stride or not state.is_contiguous():
        raise RuntimeError("%s must be a contiguous uint8 tensor (..., B, %d) for K = %d, got %s %s"
                           % (what, stride, k, state.dtype, tuple(state.shape)))
    return state.shape[-2], stride


def pose_posterior_workspace(B: int, N: int, k: int, device) -> torch.Tensor | None:
    """A workspace for ``pose_posterior`` on (B, N, k): allocate it once, pass it to every call (no allocation under capture)."""
    nbytes = _lib.load().ahv_pose_posterior_workspace_bytes(B, N, _posterior_k(k))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None


def pose_posterior_state(B: int, k: int, device) -> torch.Tensor:
    """An uninitialised state for (B, k): pass it with ``reset=True`` to the first call."""
    return torch.empty((B, _lib.load().ahv_pose_posterior_state_bytes(1, _posterior_k(k))), dtype=torch.uint8, device=device)


@torch.no_grad()
def pose_posterior_finish(state: torch.Tensor, k: int, temperature: float = 0.1) -> PosePosterior:
    """The outputs of a (merged) state (``ahv_pose_posterior_finish_f32``): one launch."""
    k = _posterior_k(k)
    beta = inverse_temperature(temperature)
    B, _ = _posterior_state(state, k)
    if state.dim() != 2:
        raise RuntimeError("state must be (B, stride)")
    if not state.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % state.device)
    dev = state.device
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = PosePosterior(f(B), f(B), f(B), torch.empty((B,), dtype=torch.int64, device=dev), f(B, k), f(B), f(B, k, 3, 3), f(B, 3, 3),
                        f(B, k), f(B), state)
    _call(dev, "ahv_pose_posterior_finish_f32", state.data_ptr(), B, k, beta, *[t.data_ptr() for t in out[:10]])
    return out


@torch.no_grad()
def merge_posterior(states: torch.Tensor, k: int, temperature: float = 0.1, state: torch.Tensor | None = None,
                    reset: bool | None = None) -> torch.Tensor:
    """``states (P,B,stride)`` -> one state ``(B,stride)`` (``ahv_pose_posterior_merge``), in the order p = 0 .. P-1: what follows
    an all-gather of per-rank states.  ``state`` given: merge into it unless ``reset``."""
    k = _posterior_k(k)
    beta = inverse_temperature(temperature)
    B, stride = _posterior_state(states, k, "states")
    if states.dim() != 3:
        raise RuntimeError("states must be (P, B, stride)")
    if not states.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % states.device)
    if state is None:
        state = torch.empty((B, stride), dtype=torch.uint8, device=states.device)
        reset = True
    elif _posterior_state(state, k) != (B, stride) or state.dim() != 2 or state.device != states.device:
        raise RuntimeError("state must be a (B, stride) = %s uint8 tensor on %s" % ((B, stride), states.device))
    _call(states.device, "ahv_pose_posterior_merge", states.data_ptr(), states.shape[0], B, k, beta, state.data_ptr(),
          _lib.AHV_POSTERIOR_RESET_STATE if reset else 0)
    return state


@torch.no_grad()
def pose_posterior(scores: torch.Tensor, R: torch.Tensor, temperature: float = 0.1, anchors: torch.Tensor | None = None,
                   min_angle_deg: float | None = None, state: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                   reset: bool | None = None, symmetry=None) -> PosePosterior:
    """The posterior of ``scores (B,N)`` over the hypotheses ``R (N,3,3)`` / ``(B,N,3,3)`` at ``temperature``, bucketed by the
    ``anchors (B,K,3,3)`` (K <= 16; normally the rotations ``select_topk`` returns for a modes list; an all-zero anchor is an
    empty slot): hypothesis i counts for the FIRST anchor within ``min_angle_deg`` of it, else for the rest.  Returns a
    ``PosePosterior``: ``log_z``, ``entropy`` (nats), ``mean_score``, ``n_excluded`` (non-finite scores: they take no part),
    ``mode_prob (B,K)`` and ``rest_prob`` (summing to 1), ``mode_R_mean (B,K,3,3)`` / ``R_mean`` (the rotation nearest to the
    weighted mean matrix), ``mode_spread_deg`` / ``spread_deg``, and ``state``.  ``state`` given: this call's hypotheses are
    merged into it (chunked N) unless ``reset``, and the outputs describe the merged state.  ``workspace``: a uint8 tensor of
    ``ahv_pose_posterior_workspace_bytes`` bytes (``pose_posterior_workspace``), else a static one per shape.  Three launches;
    with ``state`` and ``workspace`` given only the outputs are allocated.  ``symmetry`` (needs anchors): the hypotheses are first
    folded with the same anchors and angle (``sym_fold``, one more launch and a (B,N,3,3) buffer), then the unchanged posterior runs
    on the folded set -- exact for the quotient: a folded hypothesis is within the angle of its anchor in the plain distance and of no
    earlier one, an unfolded one of none, so masses, mean poses and spreads are those modulo the group, and states still merge."""
    beta = inverse_temperature(temperature)
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B,N)")
    B, N = scores.shape
    if symmetry is not None:
        if anchors is None or min_angle_deg is None:
            raise RuntimeError("symmetry needs anchors and min_angle_deg")
        R = sym_fold(R, symmetry, anchors, min_angle_deg, want_info=False).R
    if anchors is None:
        k, tau = 0, 0.0
    else:
        if anchors.dim() != 4 or anchors.shape[0] != B or tuple(anchors.shape[2:]) != (3, 3):
            raise RuntimeError("anchors must be (B,K,3,3) with B = %d, got %s" % (B, tuple(anchors.shape)))
        k = _posterior_k(anchors.shape[1])
        if min_angle_deg is None:
            raise RuntimeError("min_angle_deg is required with anchors")
        tau = min_trace(min_angle_deg)
    n_rot, rstride = _rot_layout(R, B)
    if n_rot != N:
        raise RuntimeError("R holds %d hypotheses, scores %d" % (n_rot, N))
    lib = _lib.load()
    nbytes = lib.ahv_pose_posterior_workspace_bytes(B, N, k)
    if workspace is not None and workspace.numel() * workspace.element_size() < nbytes:
        raise RuntimeError("workspace of %d bytes, need %d (ahv_pose_posterior_workspace_bytes)"
                           % (workspace.numel() * workspace.element_size(), nbytes))
    tensors = (scores, R) if anchors is None else (scores, R, anchors)
    dev = _need_gpu(*tensors)
    if state is None:
        state = torch.empty((B, lib.ahv_pose_posterior_state_bytes(1, k)), dtype=torch.uint8, device=dev)
        reset = True
    elif _posterior_state(state, k)[0] != B or state.dim() != 2 or state.device != dev:
        raise RuntimeError("state must be a (B, stride) uint8 tensor for B = %d, K = %d on %s" % (B, k, dev))
    workspace, have = _workspace(_POSTERIOR_WS, (dev, B, N, k), nbytes, torch.uint8, workspace)
    s, Rc = scores.detach().contiguous(), R.detach().contiguous()
    Ac = anchors.detach().contiguous() if k else None
    _call(dev, "ahv_pose_posterior_f32", s.data_ptr(), Rc.data_ptr(), rstride, B, N, Ac.data_ptr() if k else None, k, tau, beta,
          state.data_ptr(), workspace.data_ptr() if workspace is not None else None, have,
          _lib.AHV_POSTERIOR_RESET_STATE if reset else 0)
    return pose_posterior_finish(state, k, temperature)


def verify_pair_posterior(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                          b2: torch.Tensor, k: int, min_angle_deg: float, temperature: float = 0.1, symmetry=None, **kw):
    """The verify step with distinct modes and their posterior: ``verify_pair`` with the scores kept -> ``topk_modes`` ->
    ``select_topk`` -> ``pose_posterior`` with the modes as anchors.  Returns ``verify_pair_modes``'s triple ``(mode_scores
    (B,K), mode_idx (B,K), R_modes (B,K,3,3))`` and the ``PosePosterior``; K <= 16.  ``symmetry``: modes and posterior modulo the
    group (``topk_modes`` / ``pose_posterior``).  Other keywords go to ``verify_pair``."""
    k = _posterior_k(k)
    beta = inverse_temperature(temperature)  # (checked before the first launch)
    del beta
    scores = verify_pair(vol_src, vol_tgt, R, W1, W2, b2, want_scores=True, **kw)[0]
    m_s, m_i, m_R = select_topk(topk_modes(scores, R, _topk_k(k), min_angle_deg, symmetry=symmetry), R)
    return m_s, m_i, m_R, pose_posterior(scores, R, temperature, anchors=m_R, min_angle_deg=min_angle_deg, symmetry=symmetry)


# ---- posterior resampling -----------------------------------------------------------------------------------------
# M systematic (low-variance) draws from the softmax of a score row at temperature T (``ahv_resample_f32``, include/ahv.h): draw
# j sits at (j + u) Z / M on the cumulative weights and returns the hypothesis whose interval holds it.  The draw list is
# non-decreasing, hypothesis i appears floor(M p_i) or ceil(M p_i) times, and the same inputs give the same bytes.  Rows do not
# compose across shards: gather the scores first (``dist.all_gather_scores``).

# (device, B, N) -> workspace (the tile records of one call): static like _TOPK_WS, and under the same rule
_RESAMPLE_WS = {}

ResampledVerify = collections.namedtuple(
    "ResampledVerify", ["score", "idx", "R_pred", "draws", "fine_scores", "R_fine", "coarse_scores", "coarse_key"])


def _draws(m) -> int:
    m = int(m)
    if not 1 <= m < (1 << 31):
        raise RuntimeError("M = %d draws outside 1..2^31-1" % m)
    return m


def resample_workspace(B: int, N: int, device) -> torch.Tensor | None:
    """A workspace for ``resample`` on (B, N): allocate it once, pass it to every call (no allocation under capture)."""
    nbytes = _lib.load().ahv_resample_workspace_bytes(int(B), int(N))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None


@torch.no_grad()
def resample(scores: torch.Tensor, m: int, temperature: float = 0.1, u: torch.Tensor | None = None,
             out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``m`` systematic draws per sample from the softmax of ``scores (B,N)`` at ``temperature`` (``ahv_resample_f32``): a
    non-decreasing int64 list ``(B,m)`` of hypothesis indices, hypothesis i in it ``floor(m p_i)`` or ``ceil(m p_i)`` times;
    non-finite scores are never drawn and a row without a finite score gives -1 everywhere.  ``u``: a float32 tensor ``(B,)``
    on the device, one offset in [0, 1) per sample (read on the device: a captured graph follows it), or None for 0.5; a value
    outside [0, 1) or NaN counts as 0.5.  ``out``: an int64 ``(B,m)`` tensor to write to; ``workspace``: a uint8 tensor of
    ``ahv_resample_workspace_bytes`` bytes (``resample_workspace``), else a static one per shape.  With both given the call
    allocates nothing.  Three launches."""
    if scores.dim() != 2:
        raise RuntimeError("scores must be (B,N)")
    m = _draws(m)
    beta = inverse_temperature(temperature)
    B, N = scores.shape
    if N < 1:
        raise RuntimeError("scores hold no hypothesis (N = 0)")
    if u is not None:
        if not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or tuple(u.shape) != (B,) or not u.is_contiguous():
            raise RuntimeError("u must be a contiguous float32 tensor (B,) = (%d,) on the device of scores, or None" % B)
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (B, m) or not out.is_contiguous()):
        raise RuntimeError("out must be a contiguous int64 tensor (B,M) = %s" % ((B, m),))
    nbytes = _lib.load().ahv_resample_workspace_bytes(B, N)
    if workspace is not None and workspace.numel() * workspace.element_size() < nbytes:
        raise RuntimeError("workspace of %d bytes, need %d (ahv_resample_workspace_bytes)"
                           % (workspace.numel() * workspace.element_size(), nbytes))
    dev = _need_gpu(scores) if u is None else _need_gpu(scores, u)
    if out is None:
        out = torch.empty((B, m), dtype=torch.int64, device=dev)
    elif out.device != dev:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (dev, out.device))
    if B == 0:
        return out
    workspace, have = _workspace(_RESAMPLE_WS, (dev, B, N), nbytes, torch.uint8, workspace)
    s = scores.detach().contiguous()
    _call(dev, "ahv_resample_f32", s.data_ptr(), B, N, beta, m, u.data_ptr() if u is not None else None, out.data_ptr(),
          workspace.data_ptr(), have, 0)
    return out


@torch.no_grad()
def compose_rotations_indexed(idx: torch.Tensor, R: torch.Tensor, D: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Refinement hypotheses of a draw list: ``out[b, j] = R[idx[b, j]] @ D[j]`` -> (B, M, 3, 3)
    (``ahv_compose_rotations_indexed_f32``).  ``idx (B,M)`` int64 (``resample``), R (N,3,3) or (B,N,3,3), D (M,3,3).  An index
    outside [0, N), -1 included, composes row 0 (stays in bounds, as ``compose_rotations_topk`` does: look at ``idx``)."""
    if idx.dim() != 2 or idx.dtype != torch.int64:
        raise RuntimeError("idx must be a (B,M) int64 tensor")
    if not idx.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % idx.device)
    if not idx.is_contiguous():
        raise RuntimeError("idx must be contiguous")
    B, M = idx.shape
    _need_gpu(R, D)
    if R.device != idx.device:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (idx.device, R.device))
    N, rstride = _rot_layout(R, B)
    if D.dim() != 3 or tuple(D.shape) != (M, 3, 3):
        raise RuntimeError("D must be (M,3,3) with M = %d draws, got %s" % (M, tuple(D.shape)))
    Rc, Dc = R.detach().contiguous(), D.detach().contiguous()
    if out is None:
        out = torch.empty((B, M, 3, 3), dtype=torch.float32, device=Rc.device)
    elif tuple(out.shape) != (B, M, 3, 3) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError("out must be a contiguous float32 (B, M, 3, 3) tensor")
    _call(out.device, "ahv_compose_rotations_indexed_f32", idx.data_ptr(), Rc.data_ptr(), rstride, N, Dc.data_ptr(), M, B,
          out.data_ptr())
    return out


def verify_pair_resampled(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, D: torch.Tensor, W1: torch.Tensor,
                          W2: torch.Tensor, b2: torch.Tensor, temperature: float = 0.1, u: torch.Tensor | None = None, **kw):
    """The verify step with posterior-weighted refinement: ``verify_pair`` with the scores kept -> ``resample`` (``M =
    D.shape[0]`` draws) -> ``compose_rotations_indexed`` (draw j refined by ``D[j]``) -> ``score_hypotheses`` on the draws ->
    ``select_rotation``.  Returns a ``ResampledVerify``: the fine winner ``score (B,)``, ``idx (B,)`` in [0, M) and ``R_pred
    (B,3,3)``, the draw list ``draws (B,M)``, ``fine_scores (B,M)``, the composed set ``R_fine (B,M,3,3)``, and the coarse
    ``coarse_scores (B,N)`` / arg-max ``coarse_key (B,)``.  Other keywords go to ``verify_pair``."""
    if D.dim() != 3 or tuple(D.shape[1:]) != (3, 3):
        raise RuntimeError("D must be (M,3,3)")
    m = _draws(D.shape[0])
    beta = inverse_temperature(temperature)  # (checked before the first launch)
    del beta
    s1, key1, f_tgt = verify_pair(vol_src, vol_tgt, R, W1, W2, b2, want_scores=True, want_feat_tgt=True, **kw)
    draws = resample(s1, m, temperature, u=u)
    R_fine = compose_rotations_indexed(draws, R, D)
    s2, key2 = score_hypotheses(vol_src, f_tgt, R_fine, W1, W2, b2, want_scores=True)
    score, idx, R_pred = select_rotation(key2, R_fine)
    return ResampledVerify(score, idx, R_pred, draws, s2, R_fine, s1, key1)


# ---- pose tracking ---------------------------------------------------------------------------------------------------
# The two device pieces of a particle-filter step (``ahv_track_advance`` / ``ahv_diffuse_rotations_f32``, include/ahv.h):
# advance -> ``resample`` (u) -> ``diffuse_rotations`` (reads the advanced counter) -> the scorer.  ``track.PoseTracker`` is the
# filter built on them.

def _step_counter(step, dev=None) -> torch.Tensor:
    if not isinstance(step, torch.Tensor) or step.dtype != torch.int64 or step.numel() != 1:
        raise RuntimeError("step must be an int64 tensor of ONE element on the device (it is read, and advanced, there)")
    if not step.is_cuda:
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got a tensor on %s" % step.device)
    if dev is not None and step.device != dev:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (dev, step.device))
    return step


def _angle_rad(deg, what: str, allow_none: bool = False) -> float:
    """Degrees -> radians rounded to fp32 (what the entry point takes); finite and >= 0."""
    if deg is None and allow_none:
        return 0.0
    d = float(deg)
    if not (d >= 0.0 and math.isfinite(d)):
        raise RuntimeError("%s = %r must be finite and >= 0" % (what, deg))
    try:
        return struct.unpack("f", struct.pack("f", math.radians(d)))[0]
    except OverflowError:
        raise RuntimeError("%s = %r does not fit a float32" % (what, deg)) from None


@torch.no_grad()
def track_advance(step: torch.Tensor, seed: int, batch: int, u: torch.Tensor | None = None) -> torch.Tensor:
    """Start of a tracker step (``ahv_track_advance``, one tiny launch): reads ``t = step[0]`` ON THE DEVICE, writes the
    resampling offsets ``u (batch,)`` float32 in [0, 1) -- a function of ``(seed, t + 1, b)`` -- and then ``step[0] = t + 1``.
    ``step``: an int64 tensor of one element on the device.  Returns ``u`` (pass one to allocate nothing): it goes to
    ``resample(..., u=u)`` as it is."""
    step = _step_counter(step)
    B = int(batch)
    if not 1 <= B <= 65535:
        raise RuntimeError("batch = %d outside 1..65535" % B)
    dev = step.device
    if u is None:
        u = torch.empty((B,), dtype=torch.float32, device=dev)
    elif (not isinstance(u, torch.Tensor) or u.dtype != torch.float32 or tuple(u.shape) != (B,) or not u.is_contiguous()
          or u.device != dev):
        raise RuntimeError("u must be a contiguous float32 tensor (B,) = (%d,) on %s" % (B, dev))
    _call(dev, "ahv_track_advance", int(seed) & (2**64 - 1), step.data_ptr(), B, u.data_ptr())
    return u


def _predict_args(R, idx, m, step, best_key, n_fresh, V=None):
    """What ``diffuse_rotations`` and ``predict_rotations`` (which alone has ``V``) resolve alike, after checking ``step``, ``V``,
    ``idx`` and ``n_fresh`` against ``R``: ``(dev, step, B, M, N, rstride, vstride, n_fresh)``."""
    _need_gpu(R)
    dev = R.device
    if step is None:
        raise RuntimeError("step is required: an int64 tensor of ONE element on the device")
    step = _step_counter(step, dev)
    if V is not None:
        if not isinstance(V, torch.Tensor) or V.dim() not in (2, 3) or V.shape[-1] != 3:
            raise RuntimeError("V must be (N,3) or (B,N,3), got %s" % (tuple(V.shape) if isinstance(V, torch.Tensor) else type(V),))
        _need_gpu(R, V)
    if idx is not None:
        if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.dtype != torch.int64 or not idx.is_contiguous():
            raise RuntimeError("idx must be a contiguous (B,M) int64 tensor")
        if idx.device != dev:
            raise RuntimeError("Expected all tensors to be on the same device, found %s and %s" % (dev, idx.device))
        B = idx.shape[0]
        if m is not None and int(m) != idx.shape[1]:
            raise RuntimeError("m = %d disagrees with idx %s" % (int(m), tuple(idx.shape)))
        M = idx.shape[1]
    else:
        B = (R.shape[0] if R.dim() == 4 else V.shape[0] if V is not None and V.dim() == 3
             else best_key.numel() if best_key is not None else 1)
        M = None
    N, rstride = _rot_layout(R, B)
    if N < 1:
        raise RuntimeError("R holds no rotation (N = 0)")
    vstride = 0
    if V is not None:
        if tuple(V.shape) == (B, N, 3):
            vstride = 3 * N
        elif tuple(V.shape) != (N, 3):
            raise RuntimeError("V must be (N,3) or (B,N,3) with B = %d, N = %d, got %s" % (B, N, tuple(V.shape)))
    M = _draws((N if m is None else m) if M is None else M)
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    n_fresh = int(n_fresh)
    if not 0 <= n_fresh <= M:
        raise RuntimeError("n_fresh = %d outside 0..M = %d" % (n_fresh, M))
    return dev, step, B, M, N, rstride, vstride, n_fresh


def _check_best_key(best_key, B: int, dev) -> None:
    """After the angle checks of the two predict ops, where it has always been: the first error raised stays the same."""
    if best_key is not None and (not isinstance(best_key, torch.Tensor) or best_key.dtype != torch.int64
                                 or best_key.numel() != B or best_key.device != dev or not best_key.is_contiguous()):
        raise RuntimeError("best_key must be a contiguous int64 tensor of B = %d elements on %s" % (B, dev))


def _output(t, name, shape, dev, wanted=True):
    """The float32 output ``name`` of a predict step: ``t`` checked, or a new tensor when ``t`` is None and one is ``wanted``."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32
            or t.device != dev):
        raise RuntimeError("%s must be a contiguous float32 %s = %s tensor on %s"
                           % (name, "(B, M, 3, 3)" if len(shape) == 4 else "(B, M, 3)", shape, dev))
    return t


def _refuse_overlap(sources, outputs) -> None:
    """A slot reads any row of a source, so no output may share memory with one.  ``sources``: (tensor or None, name) pairs."""
    for src, what in sources:
        if src is None:
            continue
        lo, hi = src.data_ptr(), src.data_ptr() + 4 * src.numel()
        for name, t in outputs:
            if t is not None and t.data_ptr() < hi and lo < t.data_ptr() + 4 * t.numel():
                raise RuntimeError("%s must not overlap %s (a slot reads any row of %s)" % (name, what, what))


@torch.no_grad()
def diffuse_rotations(R: torch.Tensor, idx: torch.Tensor | None = None, m: int | None = None, sigma_deg: float = 3.0,
                      step: torch.Tensor | None = None, seed: int = 0, best_key: torch.Tensor | None = None, n_fresh: int = 0,
                      max_angle_deg: float | None = None, out: torch.Tensor | None = None, want_omega: bool = False,
                      omega_out: torch.Tensor | None = None):
    """Predict step of a particle filter (``ahv_diffuse_rotations_f32``, one launch): the next particle set ``(B,M,3,3)`` from
    ``R (N,3,3)`` / ``(B,N,3,3)``.  Slot j of sample b is ``R[idx[b,j]] exp([w]x)`` with ``w = sigma z`` fresh Gaussian noise
    (``idx (B,M)`` int64 from ``resample``; None: ``j mod N`` with ``m`` slots, default N), composed as unit quaternions and
    normalised.  ``best_key (B,)`` given: slot 0 is the elite, ``R[decode(key)]`` bit for bit.  The last ``n_fresh`` slots are
    fresh Haar rotations: ``random_rotations`` at seed ``seed ^ 0x9E3779B97F4A7C15`` and offset ``(step B + b) M + j``.
    ``step``: the int64 device counter ``track_advance`` moves (read on the device: a replayed graph draws new noise); the noise
    of a slot is a function of ``(seed, step, b, j)`` alone.  ``max_angle_deg``: ``|w|`` is clipped to it (None: no limit).
    B comes from ``idx``, a per-sample ``R`` or ``best_key``, else 1.  ``want_omega``: also return ``w (B,M,3)`` as applied
    (zeros in elite and fresh slots), into ``omega_out`` (float32 ``(B,M,3)``) when one is given.  ``out`` and ``omega_out``
    must not overlap ``R``: a slot reads any row of it.  Returns ``out`` or ``(out, omega)``."""
    dev, step, B, M, N, rstride, _, n_fresh = _predict_args(R, idx, m, step, best_key, n_fresh)
    sigma = _angle_rad(sigma_deg, "sigma_deg")
    max_angle = _angle_rad(max_angle_deg, "max_angle_deg", allow_none=True)
    _check_best_key(best_key, B, dev)
    out = _output(out, "out", (B, M, 3, 3), dev)
    omega = _output(omega_out, "omega_out", (B, M, 3), dev, wanted=want_omega)
    Rc = R.detach().contiguous()
    _refuse_overlap(((Rc, "R"),), (("out", out), ("omega_out", omega)))
    _call(dev, "ahv_diffuse_rotations_f32", idx.data_ptr() if idx is not None else None, Rc.data_ptr(), rstride, N,
          best_key.data_ptr() if best_key is not None else None, M, n_fresh, B, int(seed) & (2**64 - 1), step.data_ptr(), sigma,
          max_angle, out.data_ptr(), omega.data_ptr() if omega is not None else None)
    return (out, omega) if omega is not None else out


def _unit_interval(x, what: str) -> float:
    d = float(x)
    if not 0.0 <= d <= 1.0:      # (false for NaN)
        raise RuntimeError("%s = %r must lie in [0, 1]" % (what, x))
    return d


@torch.no_grad()
def predict_rotations(R: torch.Tensor, V: torch.Tensor | None = None, idx: torch.Tensor | None = None, m: int | None = None,
                      sigma_deg: float = 3.0, sigma_vel_deg: float = 1.0, damping: float = 1.0, step: torch.Tensor | None = None,
                      seed: int = 0, best_key: torch.Tensor | None = None, coast: bool = True, n_fresh: int = 0,
                      max_angle_deg: float | None = None, max_speed_deg: float | None = None, out: torch.Tensor | None = None,
                      vel_out: torch.Tensor | None = None, want_omega: bool = False, omega_out: torch.Tensor | None = None):
    """Predict step with a constant-velocity motion model (``ahv_predict_rotations_f32``, one launch).  A particle is ``(R, v)``,
    ``v`` its body-frame rotation vector per frame: ``V (N,3)`` / ``(B,N,3)`` float32, or None for all zeros (a freshly scored
    set).  Slot j of sample b, with ``i = idx[b,j]``: ``v' = damping v_i + sigma_vel y`` (``|v'|`` clipped to ``max_speed_deg``),
    ``R_out = R_i exp([v' + w]x)`` with ``w = sigma z`` the noise ``diffuse_rotations`` draws for the same ``(seed, step, b, j)``
    (clipped to ``max_angle_deg``) and ``y`` a second, independent draw; composed as unit quaternions and normalised.
    ``best_key (B,)`` given: slot 0 is the elite, ``R`` and ``v`` of row ``decode(key)`` bit for bit, and with ``coast`` slot 1 is
    that row moved by its own velocity with no noise, ``R_n exp([v_n]x)``.  The last ``n_fresh`` slots are the Haar rotations
    ``diffuse_rotations`` writes there, with zero velocity.  Other arguments as ``diffuse_rotations``; B comes from ``idx``, a
    per-sample ``R`` or ``V``, or ``best_key``, else 1.  ``out`` / ``omega_out`` must not overlap ``R`` and ``vel_out`` must not
    overlap ``V``.  Returns ``(R_out (B,M,3,3), V_out (B,M,3))``, with ``want_omega`` / ``omega_out`` also the total rotation
    vector applied ``(B,M,3)`` (``v' + w``; ``v_n`` in the coast slot, zeros in elite and fresh slots)."""
    dev, step, B, M, N, rstride, vstride, n_fresh = _predict_args(R, idx, m, step, best_key, n_fresh, V)
    sigma = _angle_rad(sigma_deg, "sigma_deg")
    sigma_vel = _angle_rad(sigma_vel_deg, "sigma_vel_deg")
    damping = _unit_interval(damping, "damping")
    max_angle = _angle_rad(max_angle_deg, "max_angle_deg", allow_none=True)
    max_speed = _angle_rad(max_speed_deg, "max_speed_deg", allow_none=True)
    _check_best_key(best_key, B, dev)
    out = _output(out, "out", (B, M, 3, 3), dev)
    vel_out = _output(vel_out, "vel_out", (B, M, 3), dev)
    omega = _output(omega_out, "omega_out", (B, M, 3), dev, wanted=want_omega)
    Rc = R.detach().contiguous()
    Vc = V.detach().contiguous() if V is not None else None
    _refuse_overlap(((Rc, "R"), (Vc, "V")), (("out", out), ("vel_out", vel_out), ("omega_out", omega)))
    _call(dev, "ahv_predict_rotations_f32", idx.data_ptr() if idx is not None else None, Rc.data_ptr(), rstride,
          Vc.data_ptr() if Vc is not None else None, vstride, N, best_key.data_ptr() if best_key is not None else None, M,
          n_fresh, B, int(seed) & (2**64 - 1), step.data_ptr(), sigma, sigma_vel, damping, max_angle, max_speed,
          1 if coast else 0, out.data_ptr(), vel_out.data_ptr(), omega.data_ptr() if omega is not None else None)
    return (out, vel_out, omega) if omega is not None else (out, vel_out)


# ---- noise scale and fresh slots adapted on the device ---------------------------------------------------------------
# The control record (``ahv_track_control_f32`` / ``ahv_predict_rotations_ctl_f32``, include/ahv.h): ``(B,8)`` int32 words on the
# device.  ``track_control`` decides sigma, sigma_vel and n_fresh of the next frame from the innovation and the score of this
# one, ``predict_rotations_controlled`` reads them there; nothing crosses to the host, so both live inside a captured step.

TrackControl = collections.namedtuple(
    "TrackControl", ["sigma_deg", "sigma_vel_deg", "n_fresh", "lost", "reacquired", "updated", "innovation_deg", "score"])


def _control_record(control, B: int, dev) -> torch.Tensor:
    W = _lib.AHV_TRACK_CONTROL_WORDS
    if (not isinstance(control, torch.Tensor) or control.dtype != torch.int32 or tuple(control.shape) != (B, W)
            or not control.is_contiguous() or control.device != dev):
        raise RuntimeError("control must be a contiguous int32 (B, %d) = (%d, %d) tensor on %s (track_control_state)"
                           % (W, B, W, dev))
    return control


def track_control_state(B: int, sigma_deg: float, sigma_vel_deg: float, n_fresh: int, device) -> torch.Tensor:
    """A fresh control record ``(B,8)`` int32 on ``device``: ``sigma_deg``, ``sigma_vel_deg`` (radians, fp32) and ``n_fresh`` in
    words 0-2, no flags, ``m = sigma^2``, NaN for the innovation and the score.  Built on the host and copied: not for the
    inside of a captured step (``PoseTracker.init`` copies one into the record it owns)."""
    B = int(B)
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    sigma, sigma_vel = _angle_rad(sigma_deg, "sigma_deg"), _angle_rad(sigma_vel_deg, "sigma_vel_deg")
    if int(n_fresh) < 0:
        raise RuntimeError("n_fresh = %d must be >= 0" % int(n_fresh))
    f = torch.tensor([sigma, sigma_vel, 0.0, 0.0, sigma, float("nan"), float("nan"), 0.0], dtype=torch.float32)
    f[4] = f[4] * f[4]
    rec = f.view(torch.int32).clone()
    rec[2], rec[3], rec[7] = int(n_fresh), 0, 0
    return rec[None].repeat(B, 1).to(device)


def decode_track_control(control: torch.Tensor) -> TrackControl:
    """The record as a ``TrackControl`` of ``(B,)`` tensors ON THE HOST: ``sigma_deg``, ``sigma_vel_deg`` (float32),
    ``n_fresh`` (int32), ``lost``, ``reacquired``, ``updated`` (bool), ``innovation_deg`` (NaN when none was computed) and
    ``score``.  It copies the record to the host, which synchronises: for logging and tests, not for the inside of a step."""
    W = _lib.AHV_TRACK_CONTROL_WORDS
    if not isinstance(control, torch.Tensor) or control.dtype != torch.int32 or control.dim() != 2 or control.shape[1] != W:
        raise RuntimeError("control must be an int32 (B, %d) tensor, got %s"
                           % (W, tuple(control.shape) if isinstance(control, torch.Tensor) else type(control)))
    rec = control.detach().cpu().contiguous()
    f = rec.view(torch.float32)
    flags = rec[:, 3]
    bit = lambda mask: (flags & mask) != 0
    return TrackControl(torch.rad2deg(f[:, 0]), torch.rad2deg(f[:, 1]), rec[:, 2].clone(), bit(_lib.AHV_TRACK_LOST),
                        bit(_lib.AHV_TRACK_REACQUIRED), bit(_lib.AHV_TRACK_UPDATED), torch.rad2deg(f[:, 5]), f[:, 6].clone())


@functools.lru_cache(maxsize=64)
def _control_params(first, sigma_deg, sigma_vel_deg, n_fresh, sigma_min_deg, sigma_max_deg, gain, rate, score_floor, n_fresh_lost, M):
    """The by-value arguments of ``ahv_track_control_f32``, checked: ``(first, sigma0, sigma_vel0, n_fresh0, sigma_min, sigma_max,
    gain, rate, score_floor, n_fresh_lost)``, angles in fp32 radians.  Cached: a tracker passes the same eleven values every
    step, and the eager step is bound by the host."""
    if int(first) not in (1, 2):
        raise RuntimeError("first = %r must be 1, or 2 with a coast slot" % (first,))
    sigma0, sigma_vel0 = _angle_rad(sigma_deg, "sigma_deg"), _angle_rad(sigma_vel_deg, "sigma_vel_deg")
    smin, smax = _angle_rad(sigma_min_deg, "sigma_min_deg"), _angle_rad(sigma_max_deg, "sigma_max_deg")
    if not sigma0 > 0.0:
        raise RuntimeError("sigma_deg = %r must be > 0 (sigma_vel follows sigma / sigma_deg)" % (sigma_deg,))
    if not 0.0 < smin <= smax:
        raise RuntimeError("sigma_min_deg = %r and sigma_max_deg = %r: need 0 < sigma_min <= sigma_max" % (sigma_min_deg, sigma_max_deg))
    gain, rate = float(gain), float(rate)
    if not (gain > 0.0 and math.isfinite(gain)):
        raise RuntimeError("gain = %r must be finite and > 0" % (gain,))
    if not 0.0 < rate <= 1.0:
        raise RuntimeError("rate = %r outside (0, 1]" % (rate,))
    floor = -math.inf if score_floor is None else float(score_floor)
    if math.isnan(floor):
        raise RuntimeError("score_floor is NaN (None: no floor)")
    n_fresh = int(n_fresh)
    n_lost = n_fresh if n_fresh_lost is None else int(n_fresh_lost)
    for name, n in (("n_fresh", n_fresh), ("n_fresh_lost", n_lost)):
        if not 0 <= n <= M:
            raise RuntimeError("%s = %d outside 0..M = %d" % (name, n, M))
    return int(first), sigma0, sigma_vel0, n_fresh, smin, smax, gain, rate, floor, n_lost


@torch.no_grad()
def track_control(control: torch.Tensor, R: torch.Tensor, idx: torch.Tensor, score: torch.Tensor, V: torch.Tensor | None = None,
                  first: int = 1, sigma_deg: float = 3.0, sigma_vel_deg: float = 1.0, n_fresh: int = 0,
                  sigma_min_deg: float = 0.5, sigma_max_deg: float = 8.0, gain: float = 1.5, rate: float = 0.5,
                  score_floor: float | None = None, n_fresh_lost: int | None = None, reacquired: torch.Tensor | None = None):
    """The decision of an adaptive tracker step (``ahv_track_control_f32``, one launch, after ``select_rotation``): from the
    step's particle set ``R (B,M,3,3)``, its velocities ``V (B,M,3)`` or None, the winner's slot ``idx (B,)`` int64 and its
    ``score (B,)``, rewrite ``control (B,8)`` in place.  The innovation ``a`` is the angle between the winner and the pose slot
    0 -- the previous MAP pose -- coasts to; ``lost = not score >= score_floor`` (None: no floor), ``reacquired = idx >=
    max(M - n_fresh used this frame, first)``; ``m <- (1 - rate) m + rate a^2 / 3`` unless lost or reacquired; the next frame's
    ``sigma = clamp(gain sqrt(m), sigma_min, sigma_max)`` (``sigma_max`` when lost), ``sigma_vel = sigma_vel_deg sigma /
    sigma_deg`` and ``n_fresh`` (``n_fresh_lost`` when lost; None: ``n_fresh``).  ``sigma_deg``, ``sigma_vel_deg`` and
    ``n_fresh`` are the tracker's constants; ``first`` is 1, or 2 with a coast slot.  Returns ``reacquired (B,)`` bool (pass one
    to allocate nothing).  Nothing is read on the host."""
    if not isinstance(R, torch.Tensor) or R.dim() != 4 or tuple(R.shape[2:]) != (3, 3):
        raise RuntimeError("R must be (B,M,3,3), got %s" % (tuple(R.shape) if isinstance(R, torch.Tensor) else type(R),))
    dev = _need_gpu(R, score) if V is None else _need_gpu(R, score, V)
    B, M = R.shape[0], _draws(R.shape[1])
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    if V is not None and (tuple(V.shape) != (B, M, 3) or not V.is_contiguous()):
        raise RuntimeError("V must be a contiguous (B,M,3) = (%d,%d,3) tensor, got %s" % (B, M, tuple(V.shape)))
    if tuple(score.shape) != (B,) or not score.is_contiguous():
        raise RuntimeError("score must be a contiguous (B,) = (%d,) tensor, got %s" % (B, tuple(score.shape)))
    if (not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or tuple(idx.shape) != (B,) or not idx.is_contiguous()
            or idx.device != dev):
        raise RuntimeError("idx must be a contiguous int64 (B,) = (%d,) tensor on %s" % (B, dev))
    control = _control_record(control, B, dev)
    first, sigma0, sigma_vel0, n_fresh, smin, smax, gain, rate, floor, n_lost = _control_params(
        first, sigma_deg, sigma_vel_deg, n_fresh, sigma_min_deg, sigma_max_deg, gain, rate, score_floor, n_fresh_lost, M)
    if reacquired is None:
        reacquired = torch.empty((B,), dtype=torch.bool, device=dev)
    elif (not isinstance(reacquired, torch.Tensor) or reacquired.dtype != torch.bool or tuple(reacquired.shape) != (B,)
          or not reacquired.is_contiguous() or reacquired.device != dev):
        raise RuntimeError("reacquired must be a contiguous bool (B,) = (%d,) tensor on %s" % (B, dev))
    Rc = R if R.is_contiguous() else R.contiguous()
    _call(dev, "ahv_track_control_f32", Rc.data_ptr(), V.data_ptr() if V is not None else None, idx.data_ptr(), score.data_ptr(), B,
          M, int(first), sigma0, sigma_vel0, n_fresh, smin, smax, gain, rate, floor, n_lost, control.data_ptr(),
          reacquired.data_ptr())
    return reacquired


@torch.no_grad()
def predict_rotations_controlled(R: torch.Tensor, control: torch.Tensor, V: torch.Tensor | None = None,
                                 idx: torch.Tensor | None = None, m: int | None = None, damping: float = 1.0,
                                 step: torch.Tensor | None = None, seed: int = 0, best_key: torch.Tensor | None = None,
                                 coast: bool = False, max_angle_deg: float | None = None, max_speed_deg: float | None = None,
                                 out: torch.Tensor | None = None, vel_out: torch.Tensor | None = None, velocities: bool = True,
                                 want_omega: bool = False, omega_out: torch.Tensor | None = None):
    """``predict_rotations`` with ``sigma``, ``sigma_vel`` and ``n_fresh`` read ON THE DEVICE, per sample, from ``control (B,8)``
    (``ahv_predict_rotations_ctl_f32``, one launch): a replayed graph follows the record.  For a record that holds the same
    three values in every sample the outputs are the bytes of ``predict_rotations`` with them.  ``velocities=False`` (then no
    ``V``, no ``vel_out``, no ``coast``) is the random walk: the bytes of ``diffuse_rotations``, and only ``out`` (or ``(out,
    omega)``) is returned.  Other arguments and results as ``predict_rotations``."""
    dev, step, B, M, N, rstride, vstride, _ = _predict_args(R, idx, m, step, best_key, 0, V)
    control = _control_record(control, B, dev)
    damping = _unit_interval(damping, "damping")
    max_angle = _angle_rad(max_angle_deg, "max_angle_deg", allow_none=True)
    max_speed = _angle_rad(max_speed_deg, "max_speed_deg", allow_none=True)
    _check_best_key(best_key, B, dev)
    if not velocities and (V is not None or vel_out is not None or coast):
        raise RuntimeError("velocities=False is the random walk: it takes no V, no vel_out and no coast slot")
    out = _output(out, "out", (B, M, 3, 3), dev)
    vel_out = _output(vel_out, "vel_out", (B, M, 3), dev, wanted=velocities)
    omega = _output(omega_out, "omega_out", (B, M, 3), dev, wanted=want_omega)
    Rc = R.detach().contiguous()
    Vc = V.detach().contiguous() if V is not None else None
    _refuse_overlap(((Rc, "R"), (Vc, "V")), (("out", out), ("vel_out", vel_out), ("omega_out", omega)))
    ptr = lambda t: t.data_ptr() if t is not None else None
    _call(dev, "ahv_predict_rotations_ctl_f32", ptr(idx), Rc.data_ptr(), rstride, ptr(Vc), vstride, N, ptr(best_key), M,
          control.data_ptr(), B, int(seed) & (2**64 - 1), step.data_ptr(), damping, max_angle, max_speed, 1 if coast else 0,
          out.data_ptr(), ptr(vel_out), ptr(omega))
    res = (out,) + ((vel_out,) if velocities else ()) + ((omega,) if omega is not None else ())
    return res[0] if len(res) == 1 else res


# ---- trajectory smoothing ------------------------------------------------------------------------------------------
# MAP sequence estimation over the particle history (``ahv_smooth_step_f32`` / ``ahv_smooth_backtrace_f32``, include/ahv.h): a
# Viterbi step per frame into a ring of H frames, and the backtrace that reads the path out of it.

SmoothHistory = collections.namedtuple("SmoothHistory", ["R", "P", "delta", "back"])
SmoothedPath = collections.namedtuple("SmoothedPath", ["idx", "R"])


def smooth_history(B: int, M: int, H: int, device, velocities: bool = False) -> SmoothHistory:
    """The ring of ``smooth_step``: ``R (H,B,M,3,3)`` float32, ``P`` the same shape with ``velocities`` (the predicted poses),
    else None, ``delta (H,B,M)`` float32 and ``back (H,B,M)`` int32.  Not initialised: a step at ``first_step`` reads none of
    it, and ``smooth_backtrace`` never looks behind ``first_step``."""
    B, M, H = int(B), _draws(M), int(H)
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    if not 2 <= H < (1 << 31):
        raise RuntimeError("H = %d outside 2..2^31-1 (a frame and its predecessors live in different slots)" % H)
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    return SmoothHistory(f(H, B, M, 3, 3), f(H, B, M, 3, 3) if velocities else None, f(H, B, M),
                         torch.empty((H, B, M), dtype=torch.int32, device=device))


def _smooth_ring(history):
    """``(H, B, M, dev)`` of a ``SmoothHistory`` after checking its tensors against each other."""
    if not isinstance(history, SmoothHistory) or not isinstance(history.R, torch.Tensor) or history.R.dim() != 5:
        raise RuntimeError("history must be the SmoothHistory of smooth_history()")
    H, B, M = history.R.shape[:3]
    dev = _need_gpu(history.R, history.delta) if history.P is None else _need_gpu(history.R, history.P, history.delta)
    for name, t, shape, dtype in (("R", history.R, (H, B, M, 3, 3), torch.float32), ("P", history.P, (H, B, M, 3, 3), torch.float32),
                                  ("delta", history.delta, (H, B, M), torch.float32), ("back", history.back, (H, B, M), torch.int32)):
        if t is None and name == "P":
            continue
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()
                or t.device != dev):
            raise RuntimeError("history.%s must be a contiguous %s tensor %s on %s" % (name, dtype, shape, dev))
    if not (1 <= M < (1 << 31) and 1 <= B <= 65535 and 2 <= H < (1 << 31)):
        raise RuntimeError("history of H = %d, B = %d, M = %d: outside H >= 2, 1 <= B <= 65535, 1 <= M < 2^31" % (H, B, M))
    return H, B, M, dev


def _jump(jump) -> float:
    j = float(jump)
    if not j >= 0.0:      # (false for NaN; +inf is allowed: no floor)
        raise RuntimeError("jump = %r must be >= 0 (+inf: no floor)" % (jump,))
    return j


@torch.no_grad()
def smooth_step(history: SmoothHistory, R: torch.Tensor, scores: torch.Tensor, step: torch.Tensor, temperature: float,
                sigma_deg: float, jump: float = 8.0, V: torch.Tensor | None = None, damping: float = 1.0,
                first_step: int = 1) -> SmoothHistory:
    """One Viterbi step of the trajectory smoother (``ahv_smooth_step_f32``, one launch): records the frame's particle set
    ``R (B,M,3,3)`` and ``scores (B,M)`` into slot ``t mod H`` of ``history``, ``t = step[0]`` read ON THE DEVICE (the counter
    ``track_advance`` moved, so a replayed graph records into a new slot).  With predecessors (``t > first_step``) particle j gets
    ``delta_j = s_j / T + max_i [(delta_i - m) + max(-|P_i - R_j|_F^2 / (4 sigma^2), -jump)]`` and ``back_j``, the first i that
    attains it; ``P_i`` is the pose predecessor i predicts for this frame: ``R_i exp(damping v_i)`` with velocities ``V (B,M,3)``
    (the ring then has ``P``: ``smooth_history(..., velocities=True)``), else ``R_i``.  ``sigma_deg > 0`` is the scale of the
    transition (-theta^2 / (2 sigma^2) for a small angle theta) and ``jump`` the price of an arbitrary jump (+inf: none).  A
    particle whose score is not finite is dead (``delta = -inf``, ``back = -1``).  No allocation, no host synchronisation.
    Returns ``history``."""
    H, B, M, dev = _smooth_ring(history)
    _need_gpu(history.R, R, scores)
    step = _step_counter(step, dev)
    if tuple(R.shape) != (B, M, 3, 3) or tuple(scores.shape) != (B, M):
        raise RuntimeError("R must be (B,M,3,3) = %s and scores (B,M) = %s, got %s and %s"
                           % ((B, M, 3, 3), (B, M), tuple(R.shape), tuple(scores.shape)))
    if (V is not None) != (history.P is not None):
        raise RuntimeError("V and history.P go together: smooth_history(..., velocities=True) for a tracker with velocities")
    if V is not None:
        _need_gpu(history.R, V)
        if tuple(V.shape) != (B, M, 3):
            raise RuntimeError("V must be (B,M,3) = %s, got %s" % ((B, M, 3), tuple(V.shape)))
    beta = inverse_temperature(temperature)
    sigma, jump = _transition_scale(sigma_deg, jump)
    damping = _unit_interval(damping, "damping")
    Rc, sc = R.detach().contiguous(), scores.detach().contiguous()
    Vc = V.detach().contiguous() if V is not None else None
    _call(dev, "ahv_smooth_step_f32", Rc.data_ptr(), sc.data_ptr(), Vc.data_ptr() if Vc is not None else None, step.data_ptr(),
          int(first_step), B, M, H, beta, sigma, jump, damping, history.R.data_ptr(),
          history.P.data_ptr() if history.P is not None else None, history.delta.data_ptr(), history.back.data_ptr())
    return history


@torch.no_grad()
def smooth_backtrace(history: SmoothHistory, step: torch.Tensor, frames: int | None = None, first_step: int = 1,
                     out: SmoothedPath | None = None) -> SmoothedPath:
    """The MAP path over the newest ``frames`` (default H, at most H) recorded frames (``ahv_smooth_backtrace_f32``, one launch,
    one workgroup per sample): ``SmoothedPath(idx (B,F) int64, R (B,F,3,3))``, oldest first, the last column the frame of
    ``t = step[0]`` (read on the device).  ``idx[b,f]`` is the particle the path takes in that frame's set and ``R`` its pose;
    a frame before ``first_step``, and a frame without a finite delta, gives -1 and the identity, and the path restarts behind
    such a break.  ``out``: a ``SmoothedPath`` to write into (allocates nothing)."""
    H, B, M, dev = _smooth_ring(history)
    step = _step_counter(step, dev)
    F = H if frames is None else int(frames)
    if not 1 <= F <= H:
        raise RuntimeError("frames = %d outside 1..H = %d" % (F, H))
    if out is None:
        out = SmoothedPath(torch.empty((B, F), dtype=torch.int64, device=dev), torch.empty((B, F, 3, 3), dtype=torch.float32, device=dev))
    else:
        idx, Rp = out
        if (not isinstance(idx, torch.Tensor) or tuple(idx.shape) != (B, F) or idx.dtype != torch.int64 or not idx.is_contiguous()
                or idx.device != dev or not isinstance(Rp, torch.Tensor) or tuple(Rp.shape) != (B, F, 3, 3)
                or Rp.dtype != torch.float32 or not Rp.is_contiguous() or Rp.device != dev):
            raise RuntimeError("out must be SmoothedPath(int64 (B,F) = %s, float32 (B,F,3,3)), contiguous, on %s" % ((B, F), dev))
        out = SmoothedPath(idx, Rp)
    _call(dev, "ahv_smooth_backtrace_f32", history.R.data_ptr(), history.delta.data_ptr(), history.back.data_ptr(), step.data_ptr(),
          int(first_step), B, M, H, F, out.idx.data_ptr(), out.R.data_ptr())
    return out


# ---- marginal smoothing ----------------------------------------------------------------------------------------------
# Forward-backward marginals over the ring of ``smooth_step`` (``ahv_marginal_step_f32`` / ``ahv_marginal_smooth_f32``,
# include/ahv.h): the sum-product recursions of the same hidden-Markov model.  The output is a row of log-weights per frame,
# which ``pose_posterior`` takes as it is at ``temperature=1``.

MarginalHistory = collections.namedtuple("MarginalHistory", ["alpha", "emit"])
SmoothedMarginals = collections.namedtuple("SmoothedMarginals", ["logw", "idx", "R"])


def marginal_history(B: int, M: int, H: int, device) -> MarginalHistory:
    """The forward ring of ``marginal_step`` beside a ``smooth_history(B, M, H)``: ``alpha`` and ``emit``, both ``(H,B,M)``
    float32.  Not initialised: a step at ``first_step`` reads none of it and ``marginal_smooth`` never looks behind it."""
    B, M, H = int(B), _draws(M), int(H)
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    if not 2 <= H < (1 << 31):
        raise RuntimeError("H = %d outside 2..2^31-1 (a frame and its predecessors live in different slots)" % H)
    return MarginalHistory(torch.empty((H, B, M), dtype=torch.float32, device=device),
                           torch.empty((H, B, M), dtype=torch.float32, device=device))


def _marginal_ring(history, marg):
    """``(H, B, M, dev)`` of the two rings after checking them against each other."""
    if not isinstance(marg, MarginalHistory):
        raise RuntimeError("marg must be the MarginalHistory of marginal_history()")
    H, B, M, dev = _smooth_ring(history)
    for name, t in (("alpha", marg.alpha), ("emit", marg.emit)):
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != (H, B, M) or t.dtype != torch.float32 or not t.is_contiguous()
                or t.device != dev):
            raise RuntimeError("marg.%s must be a contiguous float32 tensor %s on %s (the sizes of history)" % (name, (H, B, M), dev))
    return H, B, M, dev


def _transition_scale(sigma_deg, jump):
    sigma = _angle_rad(sigma_deg, "sigma_deg")
    if not (sigma > 0.0 and 1.0 / (4.0 * sigma * sigma) < 3.0e38):
        raise RuntimeError("sigma_deg = %r must be > 0 (and 1 / (4 sigma^2) must fit a float32)" % (sigma_deg,))
    return sigma, _jump(jump)


@torch.no_grad()
def marginal_step(history: SmoothHistory, marg: MarginalHistory, R: torch.Tensor, scores: torch.Tensor, step: torch.Tensor,
                  temperature: float, sigma_deg: float, jump: float = 8.0, first_step: int = 1) -> MarginalHistory:
    """The forward step of the marginal smoother (``ahv_marginal_step_f32``, one launch) for the frame ``R (B,M,3,3)``,
    ``scores (B,M)`` and ``t = step[0]`` (read ON THE DEVICE): ``emit_j = s_j / T`` and
    ``alpha_j = emit_j + logsumexp_i [(alpha_i - m) + max(-|P_i - R_j|_F^2 / (4 sigma^2), -jump)]`` into slot ``t mod H`` of
    ``marg``; a restart (``alpha = emit``) at ``t <= first_step`` and behind a frame without a live particle; -inf for a particle
    whose score is not finite.  It READS slot ``t - 1`` of ``history.P`` (``history.R`` without velocities) and of ``marg.alpha``:
    ``smooth_step`` must have recorded the previous frame.  It WRITES slot ``t`` of ``marg`` only, so for one frame it may run
    before or after that frame's ``smooth_step``.  Same ``temperature``, ``sigma_deg``, ``jump`` and ``first_step`` as the
    ``smooth_step`` calls.  No allocation, no host synchronisation.  Returns ``marg``."""
    H, B, M, dev = _marginal_ring(history, marg)
    _need_gpu(history.R, R, scores)
    step = _step_counter(step, dev)
    if tuple(R.shape) != (B, M, 3, 3) or tuple(scores.shape) != (B, M):
        raise RuntimeError("R must be (B,M,3,3) = %s and scores (B,M) = %s, got %s and %s"
                           % ((B, M, 3, 3), (B, M), tuple(R.shape), tuple(scores.shape)))
    beta = inverse_temperature(temperature)
    sigma, jump = _transition_scale(sigma_deg, jump)
    Rc, sc = R.detach().contiguous(), scores.detach().contiguous()
    _call(dev, "ahv_marginal_step_f32", Rc.data_ptr(), sc.data_ptr(), step.data_ptr(), int(first_step), B, M, H, beta, sigma, jump,
          history.R.data_ptr(), history.P.data_ptr() if history.P is not None else None, marg.alpha.data_ptr(), marg.emit.data_ptr())
    return marg


@torch.no_grad()
def marginal_smooth(history: SmoothHistory, marg: MarginalHistory, step: torch.Tensor, sigma_deg: float, jump: float = 8.0,
                    frames: int | None = None, first_step: int = 1, out: SmoothedMarginals | None = None) -> SmoothedMarginals:
    """The smoothed marginals of the newest ``frames`` (default H, at most H) recorded frames (``ahv_marginal_smooth_f32``: the
    backward recursion, ``frames - 1`` launches, and a finish launch, issued by one call): ``SmoothedMarginals(logw (B,F,M), idx
    (B,F) int64, R (B,F,3,3))``, oldest first, the last column the frame of ``t = step[0]`` (read on the device).  ``logw[b,f]`` is
    ``log gamma``, the log-probability that the trajectory passes through each particle of that frame given all F frames (-inf
    for a dead particle; ``exp`` sums to 1) -- a score row for ``pose_posterior`` at ``temperature=1``; ``idx`` its first arg-max
    and ``R`` that particle's pose.  A frame before ``first_step`` and a frame without a live particle give -inf, -1 and the
    identity.  ``sigma_deg`` and ``jump`` as given to ``marginal_step``.  ``out``: a ``SmoothedMarginals`` to write into
    (allocates nothing)."""
    H, B, M, dev = _marginal_ring(history, marg)
    step = _step_counter(step, dev)
    F = H if frames is None else int(frames)
    if not 1 <= F <= H:
        raise RuntimeError("frames = %d outside 1..H = %d" % (F, H))
    sigma, jump = _transition_scale(sigma_deg, jump)
    if out is None:
        out = SmoothedMarginals(torch.empty((B, F, M), dtype=torch.float32, device=dev),
                                torch.empty((B, F), dtype=torch.int64, device=dev),
                                torch.empty((B, F, 3, 3), dtype=torch.float32, device=dev))
    else:
        ok = isinstance(out, tuple) and len(out) == 3
        for t, shape, dtype in zip(out if ok else (), ((B, F, M), (B, F), (B, F, 3, 3)), (torch.float32, torch.int64, torch.float32)):
            ok = ok and (isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
                         and t.device == dev)
        if not ok:
            raise RuntimeError("out must be SmoothedMarginals(float32 (B,F,M) = %s, int64 (B,F), float32 (B,F,3,3)), contiguous, on %s"
                               % ((B, F, M), dev))
        out = SmoothedMarginals(*out)
    _call(dev, "ahv_marginal_smooth_f32", history.R.data_ptr(), history.P.data_ptr() if history.P is not None else None,
          marg.alpha.data_ptr(), marg.emit.data_ptr(), step.data_ptr(), int(first_step), B, M, H, F, sigma, jump, out.logw.data_ptr(),
          out.idx.data_ptr(), out.R.data_ptr())
    return out


# ---- multi-view verification ---------------------------------------------------------------------------------------
# V posed reference views of one object (absolute rotations A_v), one query whose absolute rotation is wanted, N hypotheses Q_n
# of it: view v sees hypothesis n as R_{v,n} = Q_n A_v^T (gt_src_2_tgt_R = R_tgt R_src^-1), and the per-view scores are fused
# into ONE (B,N) row -- S_n, the weighted mean over the participating views -- and one packed key (``ahv_fuse_view_scores_f32``,
# include/ahv.h).

def _view_poses(A: torch.Tensor, Q: torch.Tensor):
    """``(B, V, N, q_batch_stride)`` of reference poses ``A (B,V,3,3)`` and hypotheses ``Q (N,3,3)`` / ``(B,N,3,3)``."""
    if A.dim() != 4 or tuple(A.shape[2:]) != (3, 3):
        raise RuntimeError("A must be (B,V,3,3), got %s" % (tuple(A.shape),))
    B, V = A.shape[:2]
    if not 1 <= V <= _lib.AHV_VIEWS_MAX:
        raise RuntimeError("V = %d outside 1..%d" % (V, _lib.AHV_VIEWS_MAX))
    if Q.dim() == 3 and tuple(Q.shape[1:]) == (3, 3):
        return B, V, Q.shape[0], 0
    if Q.dim() == 4 and Q.shape[0] == B and tuple(Q.shape[2:]) == (3, 3):
        return B, V, Q.shape[1], Q.shape[1] * 9
    raise RuntimeError("Q must be (N,3,3) or (B,N,3,3) with B = %d, got %s" % (B, tuple(Q.shape)))


def _view_weights(weights, V: int):
    """The per-view weights as V host floats (they travel in the kernel's arguments), or None for all ones."""
    if weights is None:
        return None
    if isinstance(weights, torch.Tensor):
        if weights.is_cuda:
            raise RuntimeError("weights are host values (a sequence or a CPU tensor of V floats): they are passed in the kernel's "
                               "arguments, and reading them from the GPU would synchronise")
        weights = weights.detach().reshape(-1).tolist()
    w = [float(x) for x in weights]
    if len(w) != V:
        raise RuntimeError("weights must hold V = %d values, got %d" % (V, len(w)))
    import ctypes
    return (ctypes.c_float * V)(*w)


def view_rotations(Q: torch.Tensor, A: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out[b, v, n] = Q[n] @ A[b, v].T`` -> (B,V,N,3,3) (``ahv_view_rotations_f32``): hypothesis n of the query's rotation as
    the relative rotation reference view v would see.  Q (N,3,3) shared by the batch or (B,N,3,3); A (B,V,3,3).  Reshaped to
    (B*V,N,3,3) it is the per-sample rotation set of ``score_hypotheses`` for the B*V (view, query) samples."""
    _refuse_grad("view_rotations", Q, A)
    B, V, N, qstride = _view_poses(A, Q)
    dev = _need_gpu(Q, A)
    Qc, Ac = Q.detach().contiguous(), A.detach().contiguous()
    if out is None:
        out = torch.empty((B, V, N, 3, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, V, N, 3, 3) or not out.is_contiguous() or out.device != dev or out.dtype != torch.float32:
        raise RuntimeError("out must be a contiguous float32 (B,V,N,3,3) tensor on %s" % dev)
    _call(dev, "ahv_view_rotations_f32", Qc.data_ptr(), qstride, Ac.data_ptr(), B, V, N, out.data_ptr())
    return out


def fuse_view_scores(scores: torch.Tensor, Q: torch.Tensor, A: torch.Tensor, weights=None, max_view_angle_deg: float | None = None,
                     n_offset: int = 0, want_scores: bool = True, best_key: torch.Tensor | None = None,
                     reset_best: bool | None = None):
    """Per-view scores ``(B,V,N)`` -> ``(fused (B,N) or None, best_key (B,) int64)`` in ONE launch (``ahv_fuse_view_scores_f32``):
    ``S_n = sum_v g w_v s_{v,n} / sum_v g w_v`` over the participating views, in the order v = 0 .. V-1 in fp32; -inf where no
    view participates.  ``weights``: V host floats (finite, >= 0, not all zero; None = ones); a view with weight 0 is absent
    and its scores are never read.  ``max_view_angle_deg``: view v takes part in hypothesis n only where the relative rotation
    ``Q[n] @ A[b, v].T`` is within that angle (``min_trace``'s rule; a NaN trace does not take part); None = no limit, and Q
    and A are then only checked for their shapes.  ``best_key`` given: the packed key of ``(S_n, n_offset + n)`` is merged into it
    (chunked N, shards) unless ``reset_best``; else a fresh key is returned.  Decode with ``select_rotation(key, Q)``.
    The fused row is an ordinary (B,N) score row with ``Q`` as its matrices: ``topk``, ``topk_modes`` and ``pose_posterior``
    take it unchanged, and as a weighted mean of cosine similarities it stays in [-1, 1], so a temperature means what it means
    for one pair.  Inference only."""
    _refuse_grad("fuse_view_scores", scores, Q, A)
    B, V, N, qstride = _view_poses(A, Q)
    if scores.dim() != 3 or tuple(scores.shape) != (B, V, N):
        raise RuntimeError("scores must be (B,V,N) = %s, got %s" % ((B, V, N), tuple(scores.shape)))
    w = _view_weights(weights, V)
    flags = 0
    if max_view_angle_deg is None:
        flags |= _lib.AHV_VIEWS_NO_ANGLE_LIMIT
        tau = 0.0
    else:
        tau = min_trace(max_view_angle_deg)
    dev = _need_gpu(scores, Q, A)
    if best_key is None:
        best_key = torch.empty((B,), dtype=torch.int64, device=dev)
        reset_best = True
    elif best_key.dtype != torch.int64 or best_key.numel() != B or best_key.device != dev or not best_key.is_contiguous():
        raise RuntimeError("best_key must be a contiguous int64 tensor of B = %d elements on %s" % (B, dev))
    if reset_best:
        flags |= _lib.AHV_VIEWS_RESET_BEST
    s, Qc, Ac = scores.detach().contiguous(), Q.detach().contiguous(), A.detach().contiguous()
    fused = torch.empty((B, N), dtype=torch.float32, device=dev) if want_scores else None
    _call(dev, "ahv_fuse_view_scores_f32", s.data_ptr(), Qc.data_ptr(), qstride, Ac.data_ptr(), w, B, V, N, n_offset, tau,
          fused.data_ptr() if want_scores else None, best_key.data_ptr(), flags)
    return fused, best_key


def verify_views(vol_refs: torch.Tensor, vol_query: torch.Tensor, Q: torch.Tensor, A: torch.Tensor, W1: torch.Tensor,
                 W2: torch.Tensor, b2: torch.Tensor, weights=None, max_view_angle_deg: float | None = None, n_offset: int = 0,
                 want_scores: bool = True, best_key: torch.Tensor | None = None, reset_best: bool | None = None,
                 split_f16: bool | None = None, want_view_scores: bool = False, compact: bool = False,
                 capacity: int | None = None, want_counts: bool = False):
    """The verify step against V posed reference views: ``vol_refs (B,V,16,8,8,8)`` with absolute rotations ``A (B,V,3,3)``,
    the query volume ``vol_query (B,16,8,8,8)``, hypotheses ``Q (N,3,3)`` / ``(B,N,3,3)`` of the QUERY's absolute rotation.
    ``view_rotations`` -> ONE scoring launch over the B*V (view, query) samples -> ``fuse_view_scores``.  Returns ``(fused (B,N)
    or None, best_key (B,))`` and, with ``want_view_scores``, the per-view scores ``(B,V,N)`` as third element; keywords as
    ``fuse_view_scores``, ``split_f16`` as ``score_hypotheses``.  ``select_rotation(best_key, Q)`` decodes the pose, and the fused
    row goes to ``topk`` / ``topk_modes`` / ``pose_posterior`` with ``Q`` unchanged.
    The scoring launch is ``verify_pair``'s (the query's features are built inside it, per sample, from the query volume repeated
    per view), so at V = 1 and A = I the fused row is ``verify_pair``'s score row bit for bit.  Inference only.
    ``compact=True`` (needs ``max_view_angle_deg``): only the (view, hypothesis) pairs the angle limit lets take part are composed
    and scored -- ``view_rotations_compact`` -> the same scoring launch over ``(B*V, M)`` -> ``fuse_view_scores_compact``; the
    fused row and the key are the dense call's bit for bit.  ``capacity=None``: M is the largest count, read on the host (ONE
    synchronisation); ``capacity=M``: no host read (graph-capturable), and a pair past its view's M-th is not scored and does
    not take part (``want_counts=True`` appends ``counts (B,V)`` int64, unclipped, as the last element: compare it with M).
    ``want_view_scores`` then gives ``(B,V,N)`` with NaN at every pair that was not scored."""
    _refuse_grad("verify_views", vol_refs, vol_query, Q, A, W1, W2, b2)
    if compact:
        return _verify_views_compact(vol_refs, vol_query, Q, A, W1, W2, b2, weights, max_view_angle_deg, n_offset, want_scores,
                                     best_key, reset_best, split_f16, want_view_scores, capacity, want_counts)
    if capacity is not None or want_counts:
        raise RuntimeError("capacity and want_counts belong to compact=True")
    B, V, N, _ = _view_poses(A, Q)
    if vol_refs.dim() != 6 or tuple(vol_refs.shape) != (B, V) + _VOL:
        raise RuntimeError("vol_refs must be (B,V,16,8,8,8) = %s, got %s" % ((B, V) + _VOL, tuple(vol_refs.shape)))
    if tuple(vol_query.shape) != (B,) + _VOL:
        raise RuntimeError("vol_query must be (B,16,8,8,8) with B = %d, got %s" % (B, tuple(vol_query.shape)))
    _view_weights(weights, V)  # (weights and angle are checked before the first launch)
    if max_view_angle_deg is not None:
        min_trace(max_view_angle_deg)
    dev = _need_gpu(vol_refs, vol_query, Q, A, W1, W2, b2)
    split = bool(_SPLIT_F16.get() if split_f16 is None else split_f16)
    with torch.no_grad():
        Rv = view_rotations(Q, A).reshape(B * V, N, 3, 3)
        vq = vol_query.detach()[:, None].expand((B, V) + _VOL).reshape((B * V,) + _VOL)
        feat = torch.empty((B * V, 32, 64), dtype=torch.float32, device=dev) if split else None
        view_scores, _ = _score_hypotheses_nograd(vol_refs.detach().reshape((B * V,) + _VOL), vq, Rv, W1, W2, b2, 0, True, None,
                                                  None, split, None, tgt_is_volume=True, feat_tgt_out=feat)
        view_scores = view_scores.reshape(B, V, N)
        fused, key = fuse_view_scores(view_scores, Q, A, weights, max_view_angle_deg, n_offset, want_scores, best_key,
                                      reset_best)
    return (fused, key, view_scores) if want_view_scores else (fused, key)


# ---- angle-limited multi-view verification, compact -------------------------------------------------------------
# Under an angle limit only a share of the V N pairs takes part (Haar hypotheses: ``haar_view_fraction``); the compact path
# composes and scores those alone and fuses through a slot map (``ahv_view_rotations_compact_f32``, include/ahv.h).

def haar_view_fraction(max_view_angle_deg) -> float:
    """``(theta - sin theta) / pi``: the share of Haar-uniform rotations within ``theta`` of any fixed rotation (0.182 at 90
    degrees, 0.058 at 60) -- the expected ``counts / N`` of ``view_rotations_compact`` on a Haar set, for sizing ``capacity``."""
    theta = math.radians(float(max_view_angle_deg))
    if not 0.0 <= theta <= math.pi:
        raise RuntimeError("max_view_angle_deg = %r outside [0, 180]" % (max_view_angle_deg,))
    return (theta - math.sin(theta)) / math.pi


def view_rotations_compact_workspace(B: int, V: int, N: int, device) -> torch.Tensor:
    """A workspace for ``view_rotations_compact`` on (B, V, N): allocate it once, pass it to every call (no allocation under
    capture)."""
    nbytes = _lib.load().ahv_view_rotations_compact_workspace_bytes(B, V, N)
    return torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=device)


def _view_capacity(capacity, N: int) -> int:
    M = int(capacity)
    if not 1 <= M <= N:
        raise RuntimeError("capacity = %r outside 1..N = %d" % (capacity, N))
    return M


def view_rotations_compact(Q: torch.Tensor, A: torch.Tensor, max_view_angle_deg: float, weights=None, capacity: int | None = None,
                           workspace: torch.Tensor | None = None):
    """The participating pairs of ``view_rotations`` under the angle limit, compacted (``ahv_view_rotations_compact_f32``) ->
    ``(R (B,V,M,3,3), slot (B,V,N) int32, counts (B,V) int64)``.  View v takes part in hypothesis n by ``fuse_view_scores``'s
    rule (weight > 0 and ``Q[n] @ A[b, v].T`` within the angle); per (b, v) those n are numbered in increasing order:
    ``slot[b, v, n]`` is that number, -1 (``AHV_VIEW_SLOT_EXCLUDED``) where the pair does not take part, -2
    (``AHV_VIEW_SLOT_OVERFLOW``) where it does but M slots were taken; ``R[b, v, m]`` equals ``view_rotations(Q, A)[b, v, n]`` bit
    for bit at the n with slot m and is the identity past the list's end; ``counts`` is never clipped to M.
    ``capacity=None``: a count-only call first, ``counts.max()`` is read on the host (ONE synchronisation), M = max(1, that).
    ``capacity=M``: no host read -- graph-capturable (pass ``workspace`` from ``view_rotations_compact_workspace``); compare
    ``counts`` with M when you choose.  Inference only."""
    _refuse_grad("view_rotations_compact", Q, A)
    B, V, N, qstride = _view_poses(A, Q)
    if max_view_angle_deg is None:
        raise RuntimeError("view_rotations_compact needs max_view_angle_deg (without a limit every pair takes part: view_rotations)")
    tau = min_trace(max_view_angle_deg)
    w = _view_weights(weights, V)
    M = None if capacity is None else _view_capacity(capacity, N)
    dev = _need_gpu(Q, A)
    nbytes = _lib.load().ahv_view_rotations_compact_workspace_bytes(B, V, N)
    if workspace is None:
        workspace = view_rotations_compact_workspace(B, V, N, dev)
    elif workspace.device != dev or workspace.dtype != torch.int32 or workspace.numel() * 4 < nbytes or not workspace.is_contiguous():
        raise RuntimeError("workspace must be a contiguous int32 tensor of at least %d elements on %s" % (nbytes // 4, dev))
    Qc, Ac = Q.detach().contiguous(), A.detach().contiguous()
    counts = torch.empty((B, V), dtype=torch.int64, device=dev)
    if M is None:
        _call(dev, "ahv_view_rotations_compact_f32", Qc.data_ptr(), qstride, Ac.data_ptr(), w, B, V, N, tau, 1, None, None,
              counts.data_ptr(), workspace.data_ptr(), workspace.numel() * 4)
        M = max(1, int(counts.max().item()))  # the one host synchronisation
    R = torch.empty((B, V, M, 3, 3), dtype=torch.float32, device=dev)
    slot = torch.empty((B, V, N), dtype=torch.int32, device=dev)
    _call(dev, "ahv_view_rotations_compact_f32", Qc.data_ptr(), qstride, Ac.data_ptr(), w, B, V, N, tau, M, R.data_ptr(),
          slot.data_ptr(), counts.data_ptr(), workspace.data_ptr(), workspace.numel() * 4)
    return R, slot, counts


def fuse_view_scores_compact(scores: torch.Tensor, slot: torch.Tensor, weights=None, n_offset: int = 0, want_scores: bool = True,
                             best_key: torch.Tensor | None = None, reset_best: bool | None = None):
    """Scores of the compacted pairs ``(B,V,M)`` and the slot map ``(B,V,N)`` of ``view_rotations_compact`` -> ``(fused (B,N) or
    None, best_key (B,) int64)`` in ONE launch (``ahv_fuse_view_scores_compact_f32``): ``fuse_view_scores`` with "view v takes
    part in hypothesis n" read from the slot map (``slot >= 0``) and its score from ``scores[b, v, slot]``; Q and A are not
    needed.  The same sums in the same order: with M >= every count, the dense call's fused row and key bit for bit.  A pair
    marked -2 (overflow) does not take part.  Other keywords as ``fuse_view_scores``.  Inference only."""
    _refuse_grad("fuse_view_scores_compact", scores)
    if scores.dim() != 3 or slot.dim() != 3 or tuple(slot.shape[:2]) != tuple(scores.shape[:2]):
        raise RuntimeError("scores must be (B,V,M) and slot (B,V,N) with one (B,V), got %s and %s"
                           % (tuple(scores.shape), tuple(slot.shape)))
    B, V, M = scores.shape
    N = slot.shape[2]
    if not 1 <= V <= _lib.AHV_VIEWS_MAX:
        raise RuntimeError("V = %d outside 1..%d" % (V, _lib.AHV_VIEWS_MAX))
    _view_capacity(M, N)
    w = _view_weights(weights, V)
    dev = _need_gpu(scores)
    if slot.device != dev or slot.dtype != torch.int32:
        raise RuntimeError("slot must be an int32 tensor on %s, got %s on %s" % (dev, slot.dtype, slot.device))
    if best_key is None:
        best_key = torch.empty((B,), dtype=torch.int64, device=dev)
        reset_best = True
    elif best_key.dtype != torch.int64 or best_key.numel() != B or best_key.device != dev or not best_key.is_contiguous():
        raise RuntimeError("best_key must be a contiguous int64 tensor of B = %d elements on %s" % (B, dev))
    flags = _lib.AHV_VIEWS_RESET_BEST if reset_best else 0
    s, sl = scores.detach().contiguous(), slot.contiguous()
    fused = torch.empty((B, N), dtype=torch.float32, device=dev) if want_scores else None
    _call(dev, "ahv_fuse_view_scores_compact_f32", s.data_ptr(), sl.data_ptr(), w, B, V, N, M, n_offset,
          fused.data_ptr() if want_scores else None, best_key.data_ptr(), flags)
    return fused, best_key


def _verify_views_compact(vol_refs, vol_query, Q, A, W1, W2, b2, weights, max_view_angle_deg, n_offset, want_scores, best_key,
                          reset_best, split_f16, want_view_scores, capacity, want_counts):
    """``verify_views(compact=True)``: the dense path's three stages on the participating pairs alone."""
    if max_view_angle_deg is None:
        raise RuntimeError("verify_views(compact=True) needs max_view_angle_deg: without an angle limit every pair takes part "
                           "and there is nothing to compact")
    B, V, N, _ = _view_poses(A, Q)
    if vol_refs.dim() != 6 or tuple(vol_refs.shape) != (B, V) + _VOL:
        raise RuntimeError("vol_refs must be (B,V,16,8,8,8) = %s, got %s" % ((B, V) + _VOL, tuple(vol_refs.shape)))
    if tuple(vol_query.shape) != (B,) + _VOL:
        raise RuntimeError("vol_query must be (B,16,8,8,8) with B = %d, got %s" % (B, tuple(vol_query.shape)))
    _view_weights(weights, V)  # (weights, angle and capacity are checked before the first launch)
    min_trace(max_view_angle_deg)
    if capacity is not None:
        _view_capacity(capacity, N)
    dev = _need_gpu(vol_refs, vol_query, Q, A, W1, W2, b2)
    split = bool(_SPLIT_F16.get() if split_f16 is None else split_f16)
    with torch.no_grad():
        Rc, slot, counts = view_rotations_compact(Q, A, max_view_angle_deg, weights, capacity)
        M = Rc.shape[2]
        vq = vol_query.detach()[:, None].expand((B, V) + _VOL).reshape((B * V,) + _VOL)
        feat = torch.empty((B * V, 32, 64), dtype=torch.float32, device=dev) if split else None
        view_scores, _ = _score_hypotheses_nograd(vol_refs.detach().reshape((B * V,) + _VOL), vq, Rc.reshape(B * V, M, 3, 3), W1, W2,
                                                  b2, 0, True, None, None, split, None, tgt_is_volume=True, feat_tgt_out=feat)
        view_scores = view_scores.reshape(B, V, M)
        fused, key = fuse_view_scores_compact(view_scores, slot, weights, n_offset, want_scores, best_key, reset_best)
        res = (fused, key)
        if want_view_scores:  # (B,V,N) through the slot map, stock torch: off the hot path
            took = slot >= 0
            full = torch.gather(view_scores, 2, slot.clamp(min=0).to(torch.int64))
            res += (torch.where(took, full, torch.full_like(full, float("nan"))),)
        if want_counts:
            res += (counts,)
    return res


# ---- the nearest views of a pose, staged --------------------------------------------------------------------------
# A tracked cloud sits within a few degrees of one pose: pick the K views nearest that pose on the device, stage their volumes
# and score against those K alone (``ahv_nearest_views_f32`` / ``ahv_gather_views_f32``, include/ahv.h).

ViewSelection = collections.namedtuple("ViewSelection", ["idx", "A"])


def _selection_k(k, V: int) -> int:
    K = int(k)
    if not 1 <= K <= V:
        raise RuntimeError("k = %r outside 1..V = %d" % (k, V))
    return K


def nearest_views(anchor: torch.Tensor, A: torch.Tensor, k: int, out: ViewSelection | None = None) -> ViewSelection:
    """The ``k`` reference views nearest ``anchor (B,3,3)`` among ``A (B,V,3,3)`` (``ahv_nearest_views_f32``, ONE launch) ->
    ``ViewSelection(idx (B,k) int32, A (B,k,3,3))``, nearest first: ranked by ``t = sum_ab anchor[a][b] A_v[a][b]``, descending,
    with the fp32 chain by which ``fuse_view_scores`` decides participation; equal ``t``: the lower v first; a NaN ``t`` behind
    every number.  ``A`` of the result holds bit copies of the chosen matrices: pass it as ``A`` to ``verify_views_staged``.
    The anchor is read on the device (no host synchronisation; a replayed graph follows a moving pose).  ``out``: a
    ``ViewSelection`` of that size to write into.  Inference only."""
    _refuse_grad("nearest_views", anchor, A)
    if A.dim() != 4 or tuple(A.shape[2:]) != (3, 3):
        raise RuntimeError("A must be (B,V,3,3), got %s" % (tuple(A.shape),))
    B, V = A.shape[:2]
    if not 1 <= V <= _lib.AHV_VIEWS_MAX:
        raise RuntimeError("V = %d outside 1..%d" % (V, _lib.AHV_VIEWS_MAX))
    K = _selection_k(k, V)
    if tuple(anchor.shape) != (B, 3, 3):
        raise RuntimeError("anchor must be (B,3,3) with B = %d, got %s" % (B, tuple(anchor.shape)))
    dev = _need_gpu(anchor, A)
    if out is None:
        out = ViewSelection(torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K, 3, 3), dtype=torch.float32, device=dev))
    elif (tuple(out.idx.shape) != (B, K) or out.idx.dtype != torch.int32 or tuple(out.A.shape) != (B, K, 3, 3)
          or out.A.dtype != torch.float32 or out.idx.device != dev or out.A.device != dev or not out.idx.is_contiguous()
          or not out.A.is_contiguous()):
        raise RuntimeError("out must be ViewSelection(idx: contiguous int32 (B,k), A: contiguous float32 (B,k,3,3)) on %s" % dev)
    _call(dev, "ahv_nearest_views_f32", anchor.detach().contiguous().data_ptr(), A.detach().contiguous().data_ptr(), B, V, K,
          out.idx.data_ptr(), out.A.data_ptr())
    return out


def gather_views(src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor | None = None, broadcast: bool = False) -> torch.Tensor:
    """``out[b, k] = src[b, idx[b, k]]`` as bit copies (``ahv_gather_views_f32``, ONE launch): ``src (B,V,...)``, ``idx (B,K)``
    int32 (a ``ViewSelection.idx``), ``out (B,K,...)``.  The trailing dimensions hold a multiple of 4 floats (a feature volume:
    8192; the encoder's inputs are as good) and ``src`` and ``out`` are contiguous and 16-byte aligned.  An index outside
    0..V-1 gives a row of zeros.  ``broadcast=True``: ``src (B,...)`` has no view axis and every k receives ``src[b]``.
    Inference only."""
    _refuse_grad("gather_views", src)
    if idx.dim() != 2:
        raise RuntimeError("idx must be (B,K), got %s" % (tuple(idx.shape),))
    B, K = idx.shape
    lead = 1 if broadcast else 2
    if src.dim() <= lead or src.shape[0] != B:
        raise RuntimeError("src must be %s with B = %d, got %s" % ("(B,...)" if broadcast else "(B,V,...)", B, tuple(src.shape)))
    V = K if broadcast else src.shape[1]
    if not 1 <= V <= _lib.AHV_VIEWS_MAX:
        raise RuntimeError("V = %d outside 1..%d" % (V, _lib.AHV_VIEWS_MAX))
    _selection_k(K, V)
    rest = tuple(src.shape[lead:])
    L = 1
    for d in rest:
        L *= int(d)
    if L < 4 or L % 4:
        raise RuntimeError("the rows of src hold L = %d floats: gather_views moves 16-byte words, L must be a positive multiple of 4" % L)
    dev = _need_gpu(src)
    if idx.device != dev or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise RuntimeError("idx must be a contiguous int32 tensor on %s, got %s on %s" % (dev, idx.dtype, idx.device))
    if not src.is_contiguous():
        raise RuntimeError("src must be contiguous (gather_views makes no copy of its own)")
    if out is None:
        out = torch.empty((B, K) + rest, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, K) + rest or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous float32 %s tensor on %s" % ((B, K) + rest, dev))
    if (src.data_ptr() | out.data_ptr()) & 15:
        raise RuntimeError("src and out must be 16-byte aligned (the rows move as 16-byte words)")
    _call(dev, "ahv_gather_views_f32", src.detach().data_ptr(), idx.data_ptr(), B, V, K, L, out.data_ptr(),
          _lib.AHV_GATHER_BROADCAST if broadcast else 0)
    return out


class verify_views_workspace:
    """What ``verify_views_staged`` needs between its launches on (B, K, N): ``R (B,K,N,3,3)``, the per-view rotations;
    ``scores (B,K,N)``, the per-view scores; ``keys (B*K,)``, the scoring launch's own keys; and, each on first use, ``query
    (B,K,16,8,8,8)``, the K-fold copy of a query volume that is shared by the views, and ``feat (B*K,32,64)``, the target
    features of the split-f16 scorer.  Allocate once, pass to every call: past the first one a call allocates nothing."""

    def __init__(self, B: int, K: int, N: int, device):
        self.B, self.K, self.N = int(B), int(K), int(N)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        self.R = f(self.B, self.K, self.N, 3, 3)
        self.scores = f(self.B, self.K, self.N)
        self.keys = torch.empty((self.B * self.K,), dtype=torch.int64, device=device)
        self.query = self.feat = None

    def shared_query(self) -> torch.Tensor:
        if self.query is None:
            self.query = torch.empty((self.B, self.K) + _VOL, dtype=torch.float32, device=self.R.device)
        return self.query

    def features(self) -> torch.Tensor:
        if self.feat is None:
            self.feat = torch.empty((self.B * self.K, 32, 64), dtype=torch.float32, device=self.R.device)
        return self.feat


def verify_views_staged(vol_refs: torch.Tensor, vol_query: torch.Tensor, Q: torch.Tensor, A_sel: torch.Tensor, W1: torch.Tensor,
                        W2: torch.Tensor, b2: torch.Tensor, max_view_angle_deg: float | None = None,
                        workspace: verify_views_workspace | None = None, scores_out: torch.Tensor | None = None,
                        best_key: torch.Tensor | None = None, reset_best: bool | None = None, split_f16: bool | None = None):
    """``verify_views`` on K staged views, with every buffer the caller's: ``vol_refs (B,K,16,8,8,8)`` with rotations ``A_sel
    (B,K,3,3)`` (a ``ViewSelection.A``), ``vol_query (B,K,16,8,8,8)`` -- one query volume per view, what an encoder that sees a
    (reference, frame) pair produces -- or ``(B,16,8,8,8)``, shared by the views; hypotheses ``Q (N,3,3)`` / ``(B,N,3,3)`` of the
    query's absolute rotation.  ``view_rotations`` into the workspace -> the scoring launch of ``verify_pair`` over the B*K
    samples -> ``fuse_view_scores`` with weights of ones.  Returns ``(fused (B,N), best_key (B,))``; with a shared query both
    are ``verify_views(vol_refs, vol_query, Q, A_sel, max_view_angle_deg=...)``'s bit for bit.
    ``workspace`` (``verify_views_workspace(B, K, N, device)``), ``scores_out (B,N)`` and ``best_key (B,)`` given: no allocation
    (graph-capturable).  ``best_key`` given: merged into unless ``reset_best``.  A hypothesis no view sees within the angle
    scores -inf.  Inference only."""
    _refuse_grad("verify_views_staged", vol_refs, vol_query, Q, A_sel, W1, W2, b2)
    B, K, N, qstride = _view_poses(A_sel, Q)
    if vol_refs.dim() != 6 or tuple(vol_refs.shape) != (B, K) + _VOL:
        raise RuntimeError("vol_refs must be (B,K,16,8,8,8) = %s, got %s" % ((B, K) + _VOL, tuple(vol_refs.shape)))
    shared = tuple(vol_query.shape) == (B,) + _VOL
    if not shared and tuple(vol_query.shape) != (B, K) + _VOL:
        raise RuntimeError("vol_query must be (B,K,16,8,8,8) or (B,16,8,8,8) with B = %d and K = %d, got %s"
                           % (B, K, tuple(vol_query.shape)))
    flags = 0
    if max_view_angle_deg is None:
        flags |= _lib.AHV_VIEWS_NO_ANGLE_LIMIT
        tau = 0.0
    else:
        tau = min_trace(max_view_angle_deg)
    dev = _need_gpu(vol_refs, vol_query, Q, A_sel, W1, W2, b2)
    ws = workspace
    if ws is None:
        ws = verify_views_workspace(B, K, N, dev)
    elif (ws.B, ws.K, ws.N) != (B, K, N) or ws.R.device != dev:
        raise RuntimeError("workspace was made for (B, K, N) = %s on %s, the call has %s on %s"
                           % ((ws.B, ws.K, ws.N), ws.R.device, (B, K, N), dev))
    if scores_out is None:
        scores_out = torch.empty((B, N), dtype=torch.float32, device=dev)
    elif (scores_out.dtype != torch.float32 or tuple(scores_out.shape) != (B, N) or not scores_out.is_contiguous()
          or scores_out.device != dev):
        raise RuntimeError("scores_out must be a contiguous float32 (B,N) = %s tensor on %s" % ((B, N), dev))
    if best_key is None:
        best_key = torch.empty((B,), dtype=torch.int64, device=dev)
        reset_best = True
    elif best_key.dtype != torch.int64 or best_key.numel() != B or best_key.device != dev or not best_key.is_contiguous():
        raise RuntimeError("best_key must be a contiguous int64 tensor of B = %d elements on %s" % (B, dev))
    if reset_best:
        flags |= _lib.AHV_VIEWS_RESET_BEST
    split = bool(_SPLIT_F16.get() if split_f16 is None else split_f16)
    with torch.no_grad():
        Qc, Ac = Q.detach().contiguous(), A_sel.detach().contiguous()
        _call(dev, "ahv_view_rotations_f32", Qc.data_ptr(), qstride, Ac.data_ptr(), B, K, N, ws.R.data_ptr())
        Rv = ws.R.view(B * K, N, 3, 3)
        vq = vol_query.detach().contiguous()
        if shared:
            copies = ws.shared_query()
            _call(dev, "ahv_gather_views_f32", vq.data_ptr(), None, B, K, K, 16 * 8 * 8 * 8, copies.data_ptr(),
                  _lib.AHV_GATHER_BROADCAST)   # the K-fold copy the scoring launch reads per sample
            vq = copies
        _score_hypotheses_nograd(vol_refs.detach().reshape((B * K,) + _VOL), vq.view((B * K,) + _VOL), Rv, W1, W2, b2, 0, True, ws.keys,
                                 True, split, None, tgt_is_volume=True, feat_tgt_out=ws.features() if split else None,
                                 scores_out=ws.scores.view(B * K, N))
        _call(dev, "ahv_fuse_view_scores_f32", ws.scores.data_ptr(), Qc.data_ptr(), qstride, Ac.data_ptr(), None, B, K, N, 0, tau,
              scores_out.data_ptr(), best_key.data_ptr(), flags)
    return scores_out, best_key


# ---- joint pose inference over an unposed image set --------------------------------------------------------------
# V images, E directed edges with an independent pairwise estimate each, all absolute rotations wanted (``ahv_pose_graph_*_f32``,
# include/ahv.h; the loop is ``posegraph.PoseGraph``).

PoseGraphInit = collections.namedtuple("PoseGraphInit", ["A", "parent_edge", "reached"])


class PoseGraphTopology:
    """The static graph of a ``PoseGraph``, validated on the host and uploaded once: ``edges`` a list of ``(i, j)`` (None: every
    ordered pair, i-major), ``root`` the gauge node.  Host side: ``n_views``, ``edges``, ``incident[k]`` = the ``(edge id,
    outgoing)`` pairs of node k in edge order, ``degree[k]`` (both directions count).  Device side, int32: ``edges_dev (E,2)``
    and ``incident_dev``, the nodes' lists one after another (``offset[k]`` where k's starts), an entry ``e |
    AHV_GRAPH_EDGE_OUTGOING`` for an edge k -> j.  A degree above ``AHV_VIEWS_MAX`` is refused: the fuse kernel takes a node's
    incident edges as its views (a complete ordered graph goes up to V = 9; larger sets need a sparser edge list)."""

    def __init__(self, n_views: int, edges=None, root: int = 0, device=None):
        V = int(n_views)
        if not 2 <= V <= _lib.AHV_GRAPH_MAX_NODES:
            raise RuntimeError("n_views = %d outside 2..%d" % (V, _lib.AHV_GRAPH_MAX_NODES))
        if edges is None:
            edges = [(i, j) for i in range(V) for j in range(V) if i != j]
        if isinstance(edges, torch.Tensor):
            edges = edges.detach().cpu().tolist()
        edges = [tuple(int(x) for x in e) for e in edges]
        if not 1 <= len(edges) <= _lib.AHV_GRAPH_MAX_EDGES:
            raise RuntimeError("%d edges: outside 1..%d" % (len(edges), _lib.AHV_GRAPH_MAX_EDGES))
        incident = [[] for _ in range(V)]
        for e, ij in enumerate(edges):
            if len(ij) != 2:
                raise RuntimeError("edge %d = %r is not a pair (i, j)" % (e, ij))
            i, j = ij
            if not (0 <= i < V and 0 <= j < V):
                raise RuntimeError("edge %d = (%d, %d) names a node outside 0..V-1 = %d" % (e, i, j, V - 1))
            if i == j:
                raise RuntimeError("edge %d = (%d, %d) is a self-loop" % (e, i, j))
            incident[i].append((e, True))
            incident[j].append((e, False))
        self.degree = [len(l) for l in incident]
        for k, d in enumerate(self.degree):
            if d > _lib.AHV_VIEWS_MAX:
                raise RuntimeError("node %d has degree %d > %d (both directions count): give a sparser edge list"
                                   % (k, d, _lib.AHV_VIEWS_MAX))
        self.root = int(root)
        if not 0 <= self.root < V:
            raise RuntimeError("root = %d outside 0..V-1 = %d" % (self.root, V - 1))
        self.n_views, self.edges, self.incident = V, edges, incident
        self.offset = [sum(self.degree[:k]) for k in range(V)]
        flat = [e | (_lib.AHV_GRAPH_EDGE_OUTGOING if out else 0) for l in incident for e, out in l]
        self.edges_dev = torch.tensor(edges, dtype=torch.int32, device=device).reshape(len(edges), 2)
        self.incident_dev = torch.tensor(flat, dtype=torch.int32, device=device)

    @property
    def n_edges(self) -> int:
        return len(self.edges)


def _graph_pairs(topology, pair_R, pair_score):
    if not isinstance(topology, PoseGraphTopology):
        raise RuntimeError("topology must be a PoseGraphTopology, got %s" % type(topology).__name__)
    E = topology.n_edges
    if pair_R.dim() != 4 or tuple(pair_R.shape[1:]) != (E, 3, 3):
        raise RuntimeError("pair_R must be (B,E,3,3) with E = %d, got %s" % (E, tuple(pair_R.shape)))
    B = pair_R.shape[0]
    if tuple(pair_score.shape) != (B, E):
        raise RuntimeError("pair_score must be (B,E) = %s, got %s" % ((B, E), tuple(pair_score.shape)))
    if not 1 <= B <= 65535:
        raise RuntimeError("B = %d outside 1..65535" % B)
    return B, E


def _graph_out(t, name, shape, dtype, dev):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous %s %s tensor on %s" % (name, str(dtype).replace("torch.", ""), shape, dev))
    return t


def _graph_device(topology, dev) -> None:
    if topology.edges_dev.device != dev:
        raise RuntimeError("Expected all tensors to be on the same device, found %s and the topology on %s"
                           % (dev, topology.edges_dev.device))


@torch.no_grad()
def pose_graph_init(pair_R: torch.Tensor, pair_score: torch.Tensor, topology: PoseGraphTopology, out=None) -> PoseGraphInit:
    """The tree start of a joint solve (``ahv_pose_graph_init_f32``, ONE launch): Prim's maximum spanning tree from
    ``topology.root`` by ``pair_score (B,E)`` (non-finite: the edge is absent; ties to the lower edge index) and the absolute
    rotations it implies from ``pair_R (B,E,3,3)``, the pairs' estimates of ``A_j A_i^T``.  Returns ``PoseGraphInit(A (B,V,3,3),
    parent_edge (B,V) int32, reached (B,V) int32)``: the root and every node it is not connected to keep the identity and a
    parent of -1.  ``out``: three tensors of those shapes to write to."""
    B, E = _graph_pairs(topology, pair_R, pair_score)
    V = topology.n_views
    dev = _need_gpu(pair_R, pair_score)
    _graph_device(topology, dev)
    A, parent, reached = (None, None, None) if out is None else out
    A = _graph_out(A, "A", (B, V, 3, 3), torch.float32, dev)
    parent = _graph_out(parent, "parent_edge", (B, V), torch.int32, dev)
    reached = _graph_out(reached, "reached", (B, V), torch.int32, dev)
    Pc, sc = pair_R.detach().contiguous(), pair_score.detach().contiguous()
    _call(dev, "ahv_pose_graph_init_f32", Pc.data_ptr(), sc.data_ptr(), topology.edges_dev.data_ptr(), B, V, E, topology.root,
          A.data_ptr(), parent.data_ptr(), reached.data_ptr())
    return PoseGraphInit(A, parent, reached)


def _graph_node(topology, k) -> int:
    k = int(k)
    if not 0 <= k < topology.n_views:
        raise RuntimeError("k = %d outside 0..V-1 = %d" % (k, topology.n_views - 1))
    return k


@torch.no_grad()
def pose_graph_propose(A: torch.Tensor, pair_R: torch.Tensor, pair_score: torch.Tensor, topology: PoseGraphTopology, k: int,
                       n: int, sigma_deg: float, sweep: int = 0, seed: int = 0, counter: torch.Tensor | None = None,
                       n_fresh: int = 0, out=None):
    """The ``n`` candidates of node k's rotation and what each incident edge makes of them (``ahv_pose_graph_propose_f32``, ONE
    launch) -> ``(Q (B,n,3,3), Rrel (B,D,n,3,3))``, D = ``topology.degree[k]``.  Slot 0 is ``A[b,k]`` bit for bit; slots 1..D what
    each incident edge implies from its neighbour's rotation and ``pair_R`` (``A[b,k]`` again where ``pair_score`` is not
    finite); the last ``n_fresh`` slots are Haar rotations; every slot between is ``A[b,k] exp([sigma z]x)`` with noise that is
    a function of ``(seed, counter, sweep, b, k, slot)`` alone.  ``counter``: the int64 device counter ``track_advance`` moves
    (read on the device; None: 0).  ``Rrel[b,d]`` is ``Q A_i^T`` for an incoming edge i -> k (the bytes of ``view_rotations``) and
    ``A_j Q^T`` for an outgoing one k -> j; ``Rrel.view(B*D, n, 3, 3)`` is the scorer's per-sample set.  ``out``: ``(Q, Rrel)``
    to write to; neither may overlap ``A``."""
    B, E = _graph_pairs(topology, pair_R, pair_score)
    V = topology.n_views
    k = _graph_node(topology, k)
    D = topology.degree[k]
    if D < 1:
        raise RuntimeError("node %d has no incident edge: nothing to propose against" % k)
    if tuple(A.shape) != (B, V, 3, 3):
        raise RuntimeError("A must be (B,V,3,3) = %s, got %s" % ((B, V, 3, 3), tuple(A.shape)))
    N, n_fresh, sweep = int(n), int(n_fresh), int(sweep)
    if n_fresh < 0:
        raise RuntimeError("n_fresh = %d must be >= 0" % n_fresh)
    if N < 1 + D + n_fresh or N >= 1 << 31:
        raise RuntimeError("n = %d candidates do not hold 1 + D + n_fresh = 1 + %d + %d slots (or n >= 2^31)" % (N, D, n_fresh))
    if not 0 <= sweep <= 255:
        raise RuntimeError("sweep = %d outside 0..255" % sweep)
    sigma = _angle_rad(sigma_deg, "sigma_deg")
    dev = _need_gpu(A, pair_R, pair_score)
    _graph_device(topology, dev)
    if counter is not None:
        _step_counter(counter, dev)
    if not A.is_contiguous():
        raise RuntimeError("A must be contiguous (pose_graph_commit writes into it)")
    Q, Rrel = (None, None) if out is None else out
    Q = _graph_out(Q, "Q", (B, N, 3, 3), torch.float32, dev)
    Rrel = _graph_out(Rrel, "Rrel", (B, D, N, 3, 3), torch.float32, dev)
    _refuse_overlap(((A, "A"),), (("Q", Q), ("Rrel", Rrel)))
    Pc, sc = pair_R.detach().contiguous(), pair_score.detach().contiguous()
    _call(dev, "ahv_pose_graph_propose_f32", A.data_ptr(), Pc.data_ptr(), sc.data_ptr(), topology.edges_dev.data_ptr(),
          topology.incident_dev.data_ptr() + 4 * topology.offset[k], B, V, E, k, D, N, n_fresh, int(seed) & (2**64 - 1),
          counter.data_ptr() if counter is not None else None, sweep, sigma, Q.data_ptr(), Rrel.data_ptr())
    return Q, Rrel


@torch.no_grad()
def pose_graph_commit(key: torch.Tensor, Q: torch.Tensor, A: torch.Tensor, node_score: torch.Tensor, k: int):
    """``A[b,k] = Q[b, decode(key[b])]`` as a bit copy and ``node_score[b,k]`` = the key's score, IN PLACE
    (``ahv_pose_graph_commit_f32``, ONE launch, no host read): ``key (B,)`` is the packed key of the fused row.  A sample whose
    key holds no finite score keeps its rotation and its score.  Returns ``(A, node_score)``."""
    if A.dim() != 4 or tuple(A.shape[2:]) != (3, 3):
        raise RuntimeError("A must be (B,V,3,3), got %s" % (tuple(A.shape),))
    B, V = A.shape[:2]
    k = int(k)
    if not 0 <= k < V:
        raise RuntimeError("k = %d outside 0..V-1 = %d" % (k, V - 1))
    if Q.dim() != 4 or Q.shape[0] != B or tuple(Q.shape[2:]) != (3, 3) or Q.shape[1] < 1:
        raise RuntimeError("Q must be (B,N,3,3) with B = %d, got %s" % (B, tuple(Q.shape)))
    if tuple(node_score.shape) != (B, V):
        raise RuntimeError("node_score must be (B,V) = %s, got %s" % ((B, V), tuple(node_score.shape)))
    dev = _need_gpu(A, Q, node_score)
    if not isinstance(key, torch.Tensor) or key.dtype != torch.int64 or key.numel() != B or key.device != dev or not key.is_contiguous():
        raise RuntimeError("key must be a contiguous int64 tensor of B = %d elements on %s" % (B, dev))
    if not (A.is_contiguous() and Q.is_contiguous() and node_score.is_contiguous()):
        raise RuntimeError("A, Q and node_score must be contiguous (A and node_score are written in place)")
    _call(dev, "ahv_pose_graph_commit_f32", key.data_ptr(), Q.data_ptr(), B, V, k, Q.shape[1], A.data_ptr(), node_score.data_ptr())
    return A, node_score


class pose_graph_workspace:
    """What ``pose_graph_score`` needs between its two launches on (B, D, N): the per-edge scores ``(B,D,N)``, the scoring
    launch's own keys ``(B*D,)`` and, on first use, the target features of the split-f16 scorer."""

    def __init__(self, B: int, D: int, N: int, device):
        self.B, self.D, self.N = int(B), int(D), int(N)
        self.scores = torch.empty((self.B, self.D, self.N), dtype=torch.float32, device=device)
        self.keys = torch.empty((self.B * self.D,), dtype=torch.int64, device=device)
        self.feat = None

    def features(self) -> torch.Tensor:
        if self.feat is None:
            self.feat = torch.empty((self.B * self.D, 32, 64), dtype=torch.float32, device=self.scores.device)
        return self.feat


def pose_graph_score(vol_src: torch.Tensor, vol_tgt: torch.Tensor, Rrel: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                     b2: torch.Tensor, weights=None, workspace: pose_graph_workspace | None = None,
                     scores_out: torch.Tensor | None = None, best_key: torch.Tensor | None = None, split_f16: bool | None = None):
    """One node's candidates against all its incident edges: the scoring launch of ``verify_pair`` over the B*D (edge) samples
    -- ``vol_src, vol_tgt (B,D,16,8,8,8)`` the staged volumes of the incident edges, ``Rrel (B,D,N,3,3)`` from
    ``pose_graph_propose`` -- and ``fuse_view_scores``' launch with no angle limit: the weighted mean over the edges in the order
    d = 0 .. D-1 in fp32 and its arg-max key, ``(fused (B,N), best_key (B,))``.  ``weights``: D host floats (None: ones; 0
    removes an edge, which is then never read).  ``workspace`` (``pose_graph_workspace(B, D, N, device)``), ``scores_out`` and
    ``best_key`` given: no allocation.  The key always starts from empty.  Inference only."""
    _refuse_grad("pose_graph_score", vol_src, vol_tgt, Rrel, W1, W2, b2)
    if Rrel.dim() != 5 or tuple(Rrel.shape[3:]) != (3, 3):
        raise RuntimeError("Rrel must be (B,D,N,3,3), got %s" % (tuple(Rrel.shape),))
    B, D, N = Rrel.shape[:3]
    if not 1 <= D <= _lib.AHV_VIEWS_MAX:
        raise RuntimeError("D = %d outside 1..%d" % (D, _lib.AHV_VIEWS_MAX))
    for name, v in (("vol_src", vol_src), ("vol_tgt", vol_tgt)):
        if tuple(v.shape) != (B, D) + _VOL:
            raise RuntimeError("%s must be (B,D,16,8,8,8) = %s, got %s" % (name, (B, D) + _VOL, tuple(v.shape)))
    w = _view_weights(weights, D)
    dev = _need_gpu(vol_src, vol_tgt, Rrel, W1, W2, b2)
    ws = workspace
    if ws is None:
        ws = pose_graph_workspace(B, D, N, dev)
    elif (ws.B, ws.D, ws.N) != (B, D, N) or ws.scores.device != dev:
        raise RuntimeError("workspace was made for (B, D, N) = %s on %s, the call has %s on %s"
                           % ((ws.B, ws.D, ws.N), ws.scores.device, (B, D, N), dev))
    scores_out = _graph_out(scores_out, "scores_out", (B, N), torch.float32, dev)
    best_key = _graph_out(best_key, "best_key", (B,), torch.int64, dev)
    split = bool(_SPLIT_F16.get() if split_f16 is None else split_f16)
    with torch.no_grad():
        _score_hypotheses_nograd(vol_src.detach().reshape((B * D,) + _VOL), vol_tgt.detach().reshape((B * D,) + _VOL),
                                 Rrel.detach().reshape(B * D, N, 3, 3), W1, W2, b2, 0, True, ws.keys, True, split, None,
                                 tgt_is_volume=True, feat_tgt_out=ws.features() if split else None,
                                 scores_out=ws.scores.view(B * D, N))
        _call(dev, "ahv_fuse_view_scores_f32", ws.scores.data_ptr(), None, 0, None, w, B, D, N, 0, 0.0, scores_out.data_ptr(),
              best_key.data_ptr(), _lib.AHV_VIEWS_NO_ANGLE_LIMIT | _lib.AHV_VIEWS_RESET_BEST)
    return scores_out, best_key


# ---- rotation gradient of the score, gradient-based pose polishing ------------------------------------------

@torch.no_grad()
def score_rotation_grad(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                        b2: torch.Tensor, grad_scores: torch.Tensor | None = None, out: torch.Tensor | None = None,
                        workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``grad_R (B,N,3,3) = grad_scores[b,n] * d score[b,n] / d R[b,n]`` (``ahv_score_rotation_grad_f32``): the Euclidean
    gradient torch.autograd returns for ``rotation_matrix`` through utils.rotate_volume -> forward_3d2d -> the mean cosine.
    R (N,3,3) shared by the batch or (B,N,3,3); a shared set still gives one gradient per sample and hypothesis.
    ``grad_scores`` None = ones.  Bitwise reproducible: ``grad_R[b,n]`` does not depend on N, on how a set is cut into
    calls or on whether the set is shared.  ``out`` / ``workspace`` (float32, ``2048*B*N`` elements): caller's buffers, so
    that a captured graph replays on the same memory."""
    if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL:
        raise RuntimeError("vol_src must be (B,16,8,8,8), got %s" % (tuple(vol_src.shape),))
    B = vol_src.shape[0]
    if tuple(feat_tgt.shape) != (B, 32, 64):
        raise RuntimeError("feat_tgt must be (B,32,64), got %s" % (tuple(feat_tgt.shape),))
    N, rstride = _rot_layout(R, B)
    tensors = (vol_src, feat_tgt, R, W1, W2, b2) + (() if grad_scores is None else (grad_scores,))
    dev = _need_gpu(*tensors)
    if grad_scores is not None and tuple(grad_scores.shape) != (B, N):
        raise RuntimeError("grad_scores must be (B,N) = %s, got %s" % ((B, N), tuple(grad_scores.shape)))
    W1c, W2c, b2c = _head(W1, W2, b2)
    vs, ft, Rc = (t.detach().contiguous() for t in (vol_src, feat_tgt, R))
    gs = None if grad_scores is None else grad_scores.detach().contiguous()
    nbytes = _lib.load().ahv_score_rotation_grad_workspace_bytes(B, N)
    if workspace is None:
        workspace = torch.empty((max(nbytes, 16) // 4,), dtype=torch.float32, device=dev)
    elif workspace.device != dev or workspace.dtype != torch.float32 or workspace.numel() * 4 < nbytes:
        raise RuntimeError("workspace must be a float32 tensor of at least %d elements on %s" % (nbytes // 4, dev))
    if out is None:
        out = torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, N, 3, 3) or not out.is_contiguous() or out.device != dev or out.dtype != torch.float32:
        raise RuntimeError("out must be a contiguous float32 (B,N,3,3) tensor on %s" % dev)
    _call(dev, "ahv_score_rotation_grad_f32", vs.data_ptr(), ft.data_ptr(), Rc.data_ptr(), rstride, W1c.data_ptr(),
          W2c.data_ptr(), b2c.data_ptr(), B, N, gs.data_ptr() if gs is not None else None, workspace.data_ptr(),
          workspace.numel() * 4, out.data_ptr())
    return out


def _ladder(ladder, dev) -> torch.Tensor:
    if isinstance(ladder, torch.Tensor):
        t = ladder.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    else:
        t = torch.tensor([float(x) for x in ladder], dtype=torch.float32, device=dev)
    if not 1 <= t.numel() <= _lib.AHV_SO3_MAX_LADDER:
        raise RuntimeError("the ladder must hold 1..%d factors" % _lib.AHV_SO3_MAX_LADDER)
    return t


def _seeds(R_cur: torch.Tensor):
    if R_cur.dim() != 4 or tuple(R_cur.shape[2:]) != (3, 3):
        raise RuntimeError("the seeds must be (B,K,3,3), got %s" % (tuple(R_cur.shape),))
    return R_cur.shape[0], _topk_k(R_cur.shape[1])


@torch.no_grad()
def so3_ascent_candidates(R_cur: torch.Tensor, grad_R: torch.Tensor, theta: torch.Tensor, ladder,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """``ahv_so3_ascent_candidates_f32``: ``R_cur, grad_R (B,K,3,3)``, ``theta (B,K)`` -> candidates ``(B, K*(L+1), 3, 3)``
    (``rotations.so3_ascent_candidates`` states the rule)."""
    B, K = _seeds(R_cur)
    dev = _need_gpu(R_cur, grad_R, theta)
    lad = _ladder(ladder, dev)
    L = lad.numel()
    if tuple(grad_R.shape) != (B, K, 3, 3) or tuple(theta.shape) != (B, K):
        raise RuntimeError("grad_R must be (B,K,3,3) and theta (B,K)")
    if out is None:
        out = torch.empty((B, K * (L + 1), 3, 3), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, K * (L + 1), 3, 3) or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous (B, K*(L+1), 3, 3) tensor")
    _call(dev, "ahv_so3_ascent_candidates_f32", R_cur.detach().contiguous().data_ptr(), grad_R.detach().contiguous().data_ptr(),
          theta.detach().contiguous().data_ptr(), lad.data_ptr(), L, B, K, out.data_ptr())
    return out


@torch.no_grad()
def so3_ascent_select(R_cand: torch.Tensor, cand_scores: torch.Tensor, ladder, R_cur: torch.Tensor, score_cur: torch.Tensor,
                      theta: torch.Tensor):
    """``ahv_so3_ascent_select_f32``: picks each seed's slot and UPDATES ``R_cur (B,K,3,3)``, ``score_cur (B,K)`` and
    ``theta (B,K)`` in place (``rotations.so3_ascent_select`` states the rule); returns the three."""
    B, K = _seeds(R_cur)
    dev = _need_gpu(R_cand, cand_scores, R_cur, score_cur, theta)
    lad = _ladder(ladder, dev)
    L = lad.numel()
    if (tuple(R_cand.shape) != (B, K * (L + 1), 3, 3) or tuple(cand_scores.shape) != (B, K * (L + 1))
            or tuple(score_cur.shape) != (B, K) or tuple(theta.shape) != (B, K)):
        raise RuntimeError("expected R_cand (B,K*(L+1),3,3), cand_scores (B,K*(L+1)), score_cur and theta (B,K)")
    for t in (R_cand, cand_scores, R_cur, score_cur, theta):
        if not t.is_contiguous():
            raise RuntimeError("so3_ascent_select works in place: its tensors must be contiguous")
    _call(dev, "ahv_so3_ascent_select_f32", R_cand.data_ptr(), cand_scores.data_ptr(), lad.data_ptr(), L, B, K,
          R_cur.data_ptr(), score_cur.data_ptr(), theta.data_ptr())
    return R_cur, score_cur, theta


def _score_into(vs, ft, Rc, W1c, W2c, b2c, scores, key) -> None:
    """The fused scorer on prepared tensors into the caller's buffers (no allocation)."""
    B, N = scores.shape
    dev = scores.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ahv_score_hypotheses_f32(vs.data_ptr(), ft.data_ptr(), Rc.data_ptr(), N * 9, 0, W1c.data_ptr(),
                                                W2c.data_ptr(), b2c.data_ptr(), B, N, scores.data_ptr(), key.data_ptr(),
                                                _lib.AHV_SCORE_RESET_BEST, _stream(dev)), "ahv_score_hypotheses_f32")


def polish_rotations(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R0: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                     b2: torch.Tensor, iters: int = 8, init_angle_deg: float = 2.0, ladder=(0.25, 0.5, 1.0, 2.0),
                     out: dict | None = None):
    """A few ascent steps on SO(3) from the seeds ``R0 (B,K,3,3)``: returns ``(R (B,K,3,3), scores (B,K), theta (B,K))``.
    Per iteration: ``score_rotation_grad`` at the seeds, ``so3_ascent_candidates`` (each seed itself + L trial angles along
    its Riemannian gradient), ONE fused-scorer launch over the ``K*(L+1)`` candidates of every sample, ``so3_ascent_select``.
    Every score compared or returned is the fused scorer's: ``scores`` equals ``score_hypotheses`` at ``R`` bit for bit, and a
    seed's score never decreases.  ``iters=0`` returns ``R0`` and its scores.  Fixed iteration count, no host
    synchronisation; with ``out`` (a dict from an earlier call of the same shapes) nothing is allocated, so the call
    replays from a hipGraph.  ``theta`` is each seed's final trust angle in radians.  Inference only."""
    _refuse_grad("polish_rotations", vol_src, feat_tgt, R0, W1, W2, b2)
    with torch.no_grad():
        if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL:
            raise RuntimeError("vol_src must be (B,16,8,8,8), got %s" % (tuple(vol_src.shape),))
        B, K = _seeds(R0)
        if vol_src.shape[0] != B or tuple(feat_tgt.shape) != (B, 32, 64):
            raise RuntimeError("expected vol_src (B,16,8,8,8), feat_tgt (B,32,64) and R0 (B,K,3,3) with one B")
        iters = int(iters)
        if iters < 0:
            raise RuntimeError("iters must be >= 0")
        dev = _need_gpu(vol_src, feat_tgt, R0, W1, W2, b2)
        W1c, W2c, b2c = _head(W1, W2, b2)
        vs, ft = vol_src.detach().contiguous(), feat_tgt.detach().contiguous()
        o = out if out is not None else {}
        # a ladder given as a device tensor is taken as it is (identified by its storage: no host read, and no host-to-
        # device copy when the first call with these buffers happens under graph capture); a sequence is copied once
        if isinstance(ladder, torch.Tensor):
            L, lad_id = ladder.numel(), ("tensor", ladder.data_ptr(), str(ladder.device), ladder.dtype)
        else:
            L, lad_id = len(ladder), tuple(float(x) for x in ladder)
        sig = (B, K, L, lad_id, float(init_angle_deg), str(dev))
        if o.get("sig") != sig:
            o.clear()
            o["sig"] = sig
            o["ladder"] = _ladder(ladder, dev)
            new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
            o["R"], o["scores"], o["theta"] = new(B, K, 3, 3), new(B, K), new(B, K)
            o["theta0"] = torch.full((B, K), math.radians(float(init_angle_deg)), dtype=torch.float32, device=dev)
            o["grad"], o["cand"], o["cand_scores"] = new(B, K, 3, 3), new(B, K * (L + 1), 3, 3), new(B, K * (L + 1))
            o["ws"] = new(max(_lib.load().ahv_score_rotation_grad_workspace_bytes(B, K), 16) // 4)
            o["key"] = new(B, dtype=torch.int64)
        R, scores, theta = o["R"], o["scores"], o["theta"]
        R.copy_(R0)
        theta.copy_(o["theta0"])
        if iters == 0:
            _score_into(vs, ft, R, W1c, W2c, b2c, scores, o["key"])
        for _ in range(iters):
            score_rotation_grad(vs, ft, R, W1c, W2c, b2c, out=o["grad"], workspace=o["ws"])
            so3_ascent_candidates(R, o["grad"], theta, o["ladder"], out=o["cand"])
            _score_into(vs, ft, o["cand"], W1c, W2c, b2c, o["cand_scores"], o["key"])
            so3_ascent_select(o["cand"], o["cand_scores"], o["ladder"], R, scores, theta)
        return R, scores, theta


def verify_pair_polished(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor,
                         b2: torch.Tensor, K: int = 8, iters: int = 8, init_angle_deg: float = 2.0,
                         ladder=(0.25, 0.5, 1.0, 2.0), **kw):
    """The verify step followed by polishing: ``verify_pair`` with the scores kept -> ``topk`` -> ``select_topk`` ->
    ``polish_rotations`` on the K best hypotheses -> the best of the K polished (first maximal).  Returns
    ``(score (B,), R_pred (B,3,3), seed_idx (B,), info)``: ``seed_idx`` is the global index of the hypothesis the winner started
    from; ``info`` holds the K-list ``topk_scores, topk_idx (B,K)`` (entry 0 is the unpolished arg-max), the list's ``keys``,
    the polished ``polished_scores (B,K)`` / ``polished_R (B,K,3,3)`` / ``theta`` and ``seed_rank (B,)``.  Other keywords go to
    ``verify_pair``, except ``split_f16``: the polishing loop scores with the fp32 scorer, and a K-list from the split-f16
    scorer beside it would break "never below the arg-max's score" -- refused (also inside ``split_f16_scorer``).  Inference
    only."""
    k = _topk_k(K)
    if kw.get("split_f16") or (kw.get("split_f16") is None and _SPLIT_F16.get()):
        raise RuntimeError("verify_pair_polished scores with the fp32 scorer throughout: split_f16 is not supported")
    scores, _key, keys, f_tgt = verify_pair_topk(vol_src, vol_tgt, R, W1, W2, b2, k, want_feat_tgt=True, **kw)
    with torch.no_grad():
        top_scores, top_idx, R_seed = select_topk(keys, R)
        Rp, sp, theta = polish_rotations(vol_src, f_tgt, R_seed, W1, W2, b2, iters=iters, init_angle_deg=init_angle_deg,
                                         ladder=ladder)
        best, rank = argmax(sp)   # first maximal (the list is in descending order of the seeds' scores)
        rows = torch.arange(sp.shape[0], device=sp.device)
        info = {"topk_scores": top_scores, "topk_idx": top_idx, "keys": keys, "polished_scores": sp, "polished_R": Rp,
                "theta": theta, "seed_rank": rank}
        return best, Rp[rows, rank], top_idx[rows, rank], info


class CoarseToFineState:
    """Scratch of ``coarse_to_fine`` for B samples on one device: the two packed keys (EMPTY between steps), the meeting
    point's counters (zero between steps) and the launch's error word.  One per caller and stream; reusing it keeps the
    step free of clearing launches."""

    def __init__(self, B: int, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got device %s" % dev)
        self.B = B
        self.keys = torch.full((2, B), _lib.AHV_KEY_EMPTY, dtype=torch.int64, device=dev)
        self.sync = torch.zeros((2 * B + 1,), dtype=torch.int32, device=dev)

    def gave_up(self) -> bool:
        """True if a workgroup of some step abandoned the meeting point (host sync).  The flag is STICKY: the kernel never
        clears it, and every later step on this state poisons its outputs (NaN / -1) too until ``clear_error()``."""
        return bool(self.sync[-1].item() != 0)

    def clear_error(self) -> None:
        """Make the state usable again after a give-up: keys back to empty, the meeting point's counters to zero (a step
        that gave up may have left them mid-count) and the error word cleared -- on the current stream, after every launch
        that used the state."""
        self.keys.fill_(_lib.AHV_KEY_EMPTY)
        self.sync.zero_()


def coarse_to_fine(vol_src: torch.Tensor, vol_tgt: torch.Tensor, R: torch.Tensor, D: torch.Tensor, W1: torch.Tensor,
                   W2: torch.Tensor, b2: torch.Tensor, state: CoarseToFineState | None = None, want_scores: bool = False,
                   want_feat_tgt: bool = False, no_teams: bool = False, spare_cus: int = 0, out: dict | None = None) -> dict:
    """BASELINE.json configs[4] on one rank as ONE launch (``ahv_coarse_to_fine_f32``): the verify step on the coarse set
    ``R (N,3,3) or (B,N,3,3)``, then -- behind a device-wide meeting point -- on the refinements ``R* @ D[n]`` of its winner,
    ``D (N2,3,3)``; the last workgroup decodes both keys.  Returns a dict with ``fine_score, fine_idx`` (index into D),
    ``R_pred (B,3,3)``, ``coarse_score, coarse_idx`` and, on request, ``coarse_scores (B,N)``, ``fine_scores (B,N2)``,
    ``feat_tgt (B,32,64)``.  ``out``: a dict from an earlier call whose tensors are written again (static buffers for
    graph capture).  With the hypothesis sets sharded over ranks use ``refine.CoarseToFine`` (five launches, two
    all-reduces).  Inference only: refuses inputs that require grad while autograd is recording."""
    _refuse_grad("coarse_to_fine", vol_src, vol_tgt, W1, W2, b2)
    with torch.no_grad():
        return _coarse_to_fine_nograd(vol_src, vol_tgt, R, D, W1, W2, b2, state, want_scores, want_feat_tgt, no_teams,
                                      spare_cus, out)


def _coarse_to_fine_nograd(vol_src, vol_tgt, R, D, W1, W2, b2, state, want_scores, want_feat_tgt, no_teams, spare_cus, out):
    if vol_src.dim() != 5 or tuple(vol_src.shape[1:]) != _VOL or tuple(vol_tgt.shape) != tuple(vol_src.shape):
        raise RuntimeError("vol_src and vol_tgt must be (B,16,8,8,8), got %s and %s" % (tuple(vol_src.shape), tuple(vol_tgt.shape)))
    B = vol_src.shape[0]
    dev = _need_gpu(vol_src, vol_tgt, R, D, W1, W2, b2)
    N, rstride = _rot_layout(R, B)
    if D.dim() != 3 or tuple(D.shape[1:]) != (3, 3):
        raise RuntimeError("D must be (N2,3,3)")
    N2 = D.shape[0]
    W1, W2, b2 = _head(W1, W2, b2)
    if state is None:
        state = CoarseToFineState(B, dev)
    elif state.B != B or state.keys.device != dev:
        raise RuntimeError("the CoarseToFineState was made for B = %d on %s" % (state.B, state.keys.device))
    vs, vt, Rc, Dc = (t.detach().contiguous() for t in (vol_src, vol_tgt, R, D))
    vt = _aligned(vt, 8)
    o = out if out is not None else {}
    def buf(name, shape, dtype=torch.float32, wanted=True):
        if not wanted:
            return None
        if name not in o:
            o[name] = torch.empty(shape, dtype=dtype, device=dev)
        return o[name]
    sc = buf("coarse_scores", (B, N), wanted=want_scores)
    sf = buf("fine_scores", (B, N2), wanted=want_scores)
    ft = buf("feat_tgt", (B, 32, 64), wanted=want_feat_tgt)
    rp, fs, cs = buf("R_pred", (B, 3, 3)), buf("fine_score", (B,)), buf("coarse_score", (B,))
    fi, ci = buf("fine_idx", (B,), torch.int64), buf("coarse_idx", (B,), torch.int64)
    p = lambda t: 0 if t is None else t.data_ptr()
    if not 0 <= spare_cus <= 255:
        raise RuntimeError("spare_cus must be in [0, 255]")
    flags = (_lib.AHV_SCORE_NO_TEAMS if no_teams else 0) | (spare_cus << _lib.AHV_SCORE_SPARE_CUS_SHIFT)
    _call(dev, "ahv_coarse_to_fine_f32", vs.data_ptr(), vt.data_ptr(), Rc.data_ptr(), rstride, N, Dc.data_ptr(), N2,
          W1.data_ptr(), W2.data_ptr(), b2.data_ptr(), B, p(sc), p(sf), state.keys.data_ptr(), state.sync.data_ptr(), p(ft),
          rp.data_ptr(), fs.data_ptr(), fi.data_ptr(), cs.data_ptr(), ci.data_ptr(), flags)
    o["state"] = state
    return o


@torch.no_grad()
def so3_grid(n_total: int, device, offset: int = 0, n: int | None = None) -> torch.Tensor:
    """Rows ``[offset, offset + n)`` of the deterministic ``n_total``-point super-Fibonacci SO(3) grid, generated on
    the device (``rotations.so3_grid_np`` is the host form of the same grid)."""
    n = n_total - offset if n is None else n
    out = torch.empty((n, 3, 3), dtype=torch.float32, device=device)
    if out.device.type != "cuda":
        raise RuntimeError("3dahv_amd ops run on the GPU only (no CPU fallback); got device %s" % out.device)
    _call(out.device, "ahv_so3_grid_f32", n_total, offset, n, out.data_ptr())
    return out


@torch.no_grad()
def random_rotations(n: int, seed: int = 0, offset: int = 0, device=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Drop-in for ``pytorch3d.transforms.random_rotations(n)`` generated on the GPU: Haar-uniform (n,3,3) fp32.
    Rotation i depends only on ``(seed, offset + i)``: ``random_rotations(n, s)[a:b]`` equals
    ``random_rotations(b - a, s, offset=a)``, so every rank can generate its own shard."""
    if out is None:
        out = torch.empty((n, 3, 3), dtype=torch.float32, device=device if device is not None else "cuda")
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n * 9:
        raise RuntimeError("out must be a contiguous float32 GPU tensor of n*9 elements")
    _call(out.device, "ahv_random_rotations_f32", seed & (2**64 - 1), offset, n, out.data_ptr())
    return out
