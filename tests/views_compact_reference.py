"""Numpy restatement of the compaction of ``ahv_view_rotations_compact_f32`` (include/ahv.h, "Angle-limited multi-view
verification, compact").  Plain module (like tests/views_reference.py, whose participation rule it takes).

Per (b, v): the participating hypotheses (``views_reference.fuse``'s g: w_v > 0 and t >= tau in fp64, a NaN t out) are numbered
in increasing n; ``slot`` holds that number where it is below ``capacity``, OVERFLOW where the pair takes part but the list was
full, EXCLUDED where it does not take part; ``counts`` is the number of participating pairs, never clipped.  The margin is
``views_reference.fuse``'s: a test compares only where it is far above what fp32 rounding moves t by.
"""
import numpy as np

from . import views_reference as vr

EXCLUDED, OVERFLOW = -1, -2


def compact(Q, A, max_view_angle_deg, weights=None, capacity=None):
    """Q (N,3,3) / (B,N,3,3), A (B,V,3,3) -> ``(slot (B,V,N) int32, counts (B,V) int64, g (B,V,N) bool, margin)``;
    ``capacity`` None = max(1, counts.max())."""
    A = np.asarray(A)
    B, V = A.shape[:2]
    N = np.asarray(Q).shape[-3]
    _, _, g, margin = vr.fuse(np.zeros((B, V, N), np.float32), Q, A, weights, max_view_angle_deg)
    counts = g.sum(axis=2).astype(np.int64)
    M = max(1, int(counts.max())) if capacity is None else int(capacity)
    assert 1 <= M <= N
    rank = np.cumsum(g, axis=2) - g                      # exclusive: the number of participating n' < n
    slot = np.where(g, np.where(rank < M, rank, OVERFLOW), EXCLUDED).astype(np.int32)
    return slot, counts, g, margin


def gather(R, slot, capacity):
    """R (B,V,N,3,3) (every pair composed) and a slot map -> (B,V,capacity,3,3): R[b,v,n] at its slot, the identity elsewhere."""
    R = np.asarray(R)
    B, V, N = slot.shape
    out = np.broadcast_to(np.eye(3, dtype=R.dtype), (B, V, capacity, 3, 3)).copy()
    b, v, n = np.nonzero(slot >= 0)
    out[b, v, slot[b, v, n]] = R[b, v, n]
    return out


def scatter(scores, slot, fill=np.nan):
    """Compact scores (B,V,M) -> (B,V,N) through the slot map, ``fill`` at every pair without a slot."""
    scores = np.asarray(scores)
    full = np.take_along_axis(scores, np.maximum(slot, 0).astype(np.int64), axis=2)
    return np.where(slot >= 0, full, np.asarray(fill, scores.dtype))
