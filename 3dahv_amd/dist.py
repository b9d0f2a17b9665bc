"""Sharding the hypothesis axis across GPUs (one process per GPU, RCCL over xGMI).

Hypotheses are independent given the per-pair constants (source volume, target
feature, head weights: 94 KB, replicated on every rank), so N is partitioned
contiguously: rank r scores [lo_r, hi_r) with ``n_offset = lo_r``.  The data
path has ONE exchange: an all-reduce(max) of B packed 64-bit keys
``(ordered_i32(score) << 32) | (0xFFFFFFFF - global_idx)``, i.e. 8*B bytes --
latency-bound, bandwidth-irrelevant.  Signed max on the key = largest score,
lowest global index among equal scores (torch.max semantics, test_co3d.py:145),
independent of how N was split.

The kernels pack the key in SIGNED int64 order (include/ahv.h, "Packed keys"), which is
what ``ReduceOp.MAX`` on an int64 tensor computes on ``nccl`` (= RCCL) and ``gloo`` alike:
the all-reduce takes the key as it is, with no re-encoding launch on either side.
"""
from __future__ import annotations

from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

KEY_EMPTY = -(1 << 63)  # AHV_KEY_EMPTY: below every real key ("nothing scored")


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced partition of range(n): sizes differ by at most one."""
    if not (0 <= rank < world):
        raise ValueError("rank %d outside world of %d" % (rank, world))
    return (n * rank) // world, (n * (rank + 1)) // world


def merge_keys(keys: torch.Tensor) -> torch.Tensor:
    """Max over dim 0 of packed int64 keys (what the all-reduce computes): (G,B) -> (B,)."""
    return keys.max(dim=0).values


def all_reduce_best(key: torch.Tensor, group=None) -> torch.Tensor:
    """In-place global merge of per-rank packed keys (B,) int64; returns ``key``."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(key, op=dist.ReduceOp.MAX, group=group)
    return key


def all_gather_topk(keys: torch.Tensor, group=None, merge_fn: Optional[Callable] = None, force: bool = False) -> torch.Tensor:
    """Global K-best list from per-rank lists ``keys (B,K)`` (packed keys, descending, EMPTY-padded: ``ops.topk``): ONE
    all-gather of ``8*B*K`` bytes per rank into ``(world,B,K)`` followed by ``ops.merge_topk`` -- the list counterpart of
    ``all_reduce_best``.  The result is the same list on every rank and does not depend on how N was cut (the keys carry
    global indices; a key met twice is kept once).  Under ``nccl`` (= RCCL) both the collective and the merge are
    capturable.  ``merge_fn`` defaults to the HIP kernel; CPU tests inject their own.  With no process group (or a world
    of one, unless ``force``) the list is returned as it is."""
    inited = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if inited else 1
    if not inited or (world == 1 and not force):
        return keys
    if merge_fn is None:
        from . import ops
        merge_fn = ops.merge_topk
    lists = torch.empty((world,) + tuple(keys.shape), dtype=keys.dtype, device=keys.device)
    # the concatenated form (world*B, K): what every backend accepts (gloo refuses the stacked shape)
    dist.all_gather_into_tensor(lists.view((-1,) + tuple(keys.shape[1:])), keys.contiguous(), group=group)
    return merge_fn(lists)


def all_gather_posterior(state: torch.Tensor, k: int, temperature: float = 0.1, group=None,
                         merge_fn: Optional[Callable] = None, force: bool = False) -> torch.Tensor:
    """Global posterior state from per-rank states ``state (B,stride)`` (uint8: ``ops.pose_posterior(...).state`` of this rank's
    shard against the SHARED anchors): ONE all-gather of the state bytes into ``(world,B,stride)`` followed by
    ``ops.merge_posterior(states, k, temperature)`` in rank order -- the same merged state on every rank, which each then
    finishes (``ops.pose_posterior_finish``).  The shape of ``all_gather_topk``: ``merge_fn`` defaults to the HIP kernel, CPU
    tests inject their own; with no process group (or a world of one, unless ``force``) the state is returned as it is."""
    inited = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if inited else 1
    if not inited or (world == 1 and not force):
        return state
    if merge_fn is None:
        from . import ops
        merge_fn = ops.merge_posterior
    states = torch.empty((world,) + tuple(state.shape), dtype=state.dtype, device=state.device)
    # the concatenated form (world*B, stride): what every backend accepts (gloo refuses the stacked shape)
    dist.all_gather_into_tensor(states.view((-1,) + tuple(state.shape[1:])), state.contiguous(), group=group)
    return merge_fn(states, k, temperature)


def all_gather_scores(scores_local: torch.Tensor, n_total: int, group=None, force: bool = False,
                      out: Optional[torch.Tensor] = None, staging: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The full score row ``(B, n_total)`` from this rank's slice ``(B, hi - lo)`` of ``shard_range(n_total, rank, world)``:
    ONE all-gather of ``4*B*ceil(n_total / world)`` bytes per rank.  What a selection that does not compose across shards
    needs (``ops.topk_modes``: a shard's local winner can suppress a hypothesis the global selection keeps): every rank then
    selects over the whole row and gets the same list bit for bit, however N was cut.  ``shard_range`` cuts unevenly, so the
    slices are padded to the largest shard and the padding is stripped.  ``out (B, n_total)`` and ``staging
    (world + 1, B, ceil(n_total / world))`` given: no allocation (capture).  With no process group (or a world of one,
    unless ``force``) the slice is returned as it is."""
    inited = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if inited else 1
    if not inited or (world == 1 and not force):
        if scores_local.shape[1] != n_total:
            raise ValueError("local scores hold %d hypotheses, expected %d" % (scores_local.shape[1], n_total))
        return scores_local
    rank = dist.get_rank(group)
    lo, hi = shard_range(n_total, rank, world)
    B = scores_local.shape[0]
    if scores_local.shape[1] != hi - lo:
        raise ValueError("local scores hold %d hypotheses, shard expects %d" % (scores_local.shape[1], hi - lo))
    width = -(-n_total // world)
    if staging is None:
        staging = torch.empty((world + 1, B, width), dtype=scores_local.dtype, device=scores_local.device)
    if out is None:
        out = torch.empty((B, n_total), dtype=scores_local.dtype, device=scores_local.device)
    mine = staging[world]
    mine[:, :hi - lo].copy_(scores_local)
    if hi - lo < width:
        mine[:, hi - lo:].zero_()
    # the concatenated form (world*B, width): what every backend accepts (gloo refuses the stacked shape)
    dist.all_gather_into_tensor(staging[:world].view(world * B, width), mine, group=group)
    for r in range(world):
        a, b = shard_range(n_total, r, world)
        out[:, a:b].copy_(staging[r, :, :b - a])
    return out


# ---- host-side key codec (numpy): used by host logic and CPU tests ------------------

def pack_keys_host(scores: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Same packing as the device code (csrc/ahv_device.h pack_key); returns int64 keys."""
    s = np.asarray(scores, dtype=np.float32) + np.float32(0.0)
    u = s.view(np.uint32).copy()
    u[np.isnan(s)] = np.uint32(0x7FC00000)
    neg = (u & np.uint32(0x80000000)) != 0
    u = np.where(neg, u ^ np.uint32(0x7FFFFFFF), u).astype(np.uint64)
    k = (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx, dtype=np.uint64))
    return k.view(np.int64)


def unpack_keys_host(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    ks = np.asarray(keys, dtype=np.int64)
    k = ks.view(np.uint64)
    u = (k >> np.uint64(32)).astype(np.uint32)
    neg = (u & np.uint32(0x80000000)) != 0
    bits = np.where(neg, u ^ np.uint32(0x7FFFFFFF), u).astype(np.uint32)
    score = bits.view(np.float32).copy()
    idx = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
    empty = ks == KEY_EMPTY
    score[empty] = -np.inf
    idx[empty] = -1
    return score, idx


# ---- sharded verify step -------------------------------------------------------------

def score_hypotheses_sharded(vol_src: torch.Tensor, feat_tgt: torch.Tensor, R: torch.Tensor, W1, W2, b2,
                             rank: Optional[int] = None, world: Optional[int] = None, group=None,
                             want_scores: bool = False, r_is_local: bool = False, n_total: Optional[int] = None,
                             score_fn: Optional[Callable] = None):
    """One verify step with N sharded over the process group.

    ``R`` is the full (N,3,3) hypothesis set present on every rank (the reference samples one
    codebook per category and reuses it, test_co3d.py:106) unless ``r_is_local``; in that case it
    is this rank's slice and ``n_total`` gives N.  Returns ``(local_scores or None, best_score (B,),
    best_idx (B,) global int64)`` -- identical on every rank.
    ``score_fn`` defaults to the HIP fused scorer; tests inject a CPU scorer to exercise the
    partition/merge logic without a GPU.
    """
    if rank is None:
        rank = dist.get_rank(group) if dist.is_initialized() else 0
    if world is None:
        world = dist.get_world_size(group) if dist.is_initialized() else 1
    if score_fn is None:
        from . import ops
        score_fn = ops.score_hypotheses
        unpack = ops.unpack_best
    else:
        unpack = None
    if r_is_local:
        if n_total is None:
            raise ValueError("n_total is required with r_is_local")
        lo, hi = shard_range(n_total, rank, world)
        R_loc = R
        if R.shape[-3] != hi - lo:
            raise ValueError("local R has %d hypotheses, shard expects %d" % (R.shape[-3], hi - lo))
    else:
        n = R.shape[-3]
        lo, hi = shard_range(n, rank, world)
        R_loc = R[..., lo:hi, :, :]
    scores, key = score_fn(vol_src, feat_tgt, R_loc.contiguous(), W1, W2, b2, n_offset=lo, want_scores=want_scores)
    key = all_reduce_best(key, group=group)
    if unpack is not None:
        best, idx = unpack(key)
    else:
        b, i = unpack_keys_host(key.cpu().numpy())
        best, idx = torch.from_numpy(b), torch.from_numpy(i)
    return scores, best, idx


def all_reduce_gradients(params: Iterable[torch.nn.Parameter], group=None, bucket_bytes: int = 64 << 20) -> int:
    """Data-parallel gradient averaging, the exchange Lightning's DDP strategy performs for the reference's
    ``trainer.fit`` (modules/model_co3d.py:101-145 with ``strategy='ddp'``, train_estimator_co3d.py:23-24).  Gradients are packed
    into flat buckets of up to ``bucket_bytes`` (the aligner has ~230 tensors / 192 MB: a few large RCCL
    all-reduces instead of hundreds of small ones), summed, divided by the world size and unpacked in place.
    Parameters without a gradient on this rank (``bn_down``) are skipped on every rank alike.  Returns the
    number of buckets.  With no process group it is a no-op."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    world = dist.get_world_size(group)
    grads = [p.grad for p in params if p.grad is not None]
    buckets, cur, size = [], [], 0
    for g in grads:
        nbytes = g.numel() * g.element_size()
        if cur and (size + nbytes > bucket_bytes or g.dtype != cur[0].dtype or g.device != cur[0].device):
            buckets.append(cur)
            cur, size = [], 0
        cur.append(g)
        size += nbytes
    if cur:
        buckets.append(cur)
    for b in buckets:
        flat = torch._utils._flatten_dense_tensors(b)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        flat.div_(world)
        for g, f in zip(b, torch._utils._unflatten_dense_tensors(flat, b)):
            g.copy_(f)
    return len(buckets)
