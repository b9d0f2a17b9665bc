"""numpy reference of posterior resampling (``ahv_resample_f32``, include/ahv.h): the exact-arithmetic definition carried out
with longdouble cumulative sums over fp64 weights of the fp32 scores, the tolerance a device result is held to, and the two
pieces an oracle-backed CPU backend needs for ``CoarseToFine(resample=True)``.

    scored set  F = { i : s_i finite }
    weights     m = max_F s_i, w_i = exp((s_i - m) beta) on F, else 0; C_i = sum_{k <= i} w_k, E_i = C_{i-1}, Z = C_{N-1}
    draws       draw j sits at t_j = (j + u) Z / M and returns the one i with E_i <= t_j < C_i

A sample without a finite score returns -1 in every slot; u outside [0, 1) (NaN included) counts as 0.5.
"""
import numpy as np

LD = np.longdouble


def beta_of(temperature):
    """1 / T in double precision, rounded to fp32: ``ops.inverse_temperature``."""
    return np.float32(1.0 / float(temperature))


def offset_of(u):
    """The offset the device uses: u as fp32 when inside [0, 1), else 0.5."""
    if u is None:
        return np.float32(0.5)
    u = np.float32(u)
    return u if (u >= 0 and u < 1) else np.float32(0.5)


def weights(s, beta):
    """fp64 weights of one row of fp32 scores (0 outside the scored set) and the mask of the scored set; None when it is empty."""
    s = np.asarray(s, dtype=np.float32)
    fin = np.isfinite(s)
    if not fin.any():
        return None, fin
    m = np.float64(s[fin].max())
    arg = (s.astype(np.float64) - m) * np.float64(beta)
    return np.where(fin, np.exp(np.where(fin, arg, 0.0)), 0.0), fin


def cdf(s, beta):
    """(p, E, C) of one row: the probabilities (fp64) and the normalised exclusive / inclusive cumulative sums (longdouble)."""
    w, _ = weights(s, beta)
    Cw = np.cumsum(w.astype(LD))
    Z = Cw[-1]
    C = Cw / Z
    E = np.concatenate([np.zeros(1, LD), C[:-1]])
    return (w / np.float64(Z)), E, C


def resample_row(s, beta, M, u=None):
    """The M draws of one row by the definition: int64 (M,)."""
    w, _ = weights(s, beta)
    if w is None:
        return np.full(M, -1, np.int64)
    C = np.cumsum(w.astype(LD))
    t = (np.arange(M, dtype=LD) + LD(offset_of(u))) * C[-1] / LD(M)
    idx = np.searchsorted(C, t, side="right")          # the first i with C_i > t_j: E_i <= t_j < C_i
    return np.minimum(idx, np.flatnonzero(w > 0)[-1]).astype(np.int64)   # (t_j < Z in exact arithmetic)


def resample_row_by_boundaries(s, beta, M, u=None):
    """The same draws stated per HYPOTHESIS, as the kernels state them: i owns the slots [h_{i-1}, h_i), h_i = clamp(ceil(C_i M
    / Z - u), 0, M) -- the number of draws below C_i --, the last one with weight forced to M, a max-scan over the integers."""
    w, _ = weights(s, beta)
    if w is None:
        return np.full(M, -1, np.int64)
    C = np.cumsum(w.astype(LD))
    h = np.clip(np.ceil(C * LD(M) / C[-1] - LD(offset_of(u))), 0, M).astype(np.int64)
    h[np.flatnonzero(w > 0)[-1]:] = M
    h = np.where(w > 0, h, 0)
    h = np.maximum.accumulate(h)
    return np.repeat(np.arange(len(w), dtype=np.int64), np.diff(np.concatenate([[0], h])))


def resample(scores, M, temperature=0.1, u=None):
    """(B,N) fp32 scores -> (B,M) int64 draws; u: None, a scalar or (B,) values."""
    scores = np.asarray(scores, dtype=np.float32)
    beta = beta_of(temperature)
    us = [None] * len(scores) if u is None else np.broadcast_to(np.asarray(u, dtype=np.float32), (len(scores),))
    return np.stack([resample_row(s, beta, M, us[b]) for b, s in enumerate(scores)])


def tolerance(s, beta):
    """eps on the NORMALISED cumulative sums for a device that takes the weights by an fp32 expf of the fp32 argument:
    2 max_F (|(s_i - m) beta| 2^-23 + 2^-22) + 1e-12.  The argument is rounded twice in fp32 (the difference, the product), which
    moves a weight by |arg| 2^-23 relative; expf is good to 2 ulp = 2^-22; numerator and denominator of the normalised sum both
    move: the factor 2.  1e-12 covers the fp64 sums.  Derived, not tuned: 2.4e-6 for scores in [-0.2, 0.6] at T = 0.1."""
    s = np.asarray(s, dtype=np.float32)
    fin = np.isfinite(s)
    if not fin.any():
        return 1e-12
    arg = np.abs((s[fin].astype(np.float64) - np.float64(s[fin].max())) * np.float64(beta))
    return float(2.0 * (arg.max() * 2.0 ** -23 + 2.0 ** -22) + 1e-12)


def check_draws(idx, s, beta, u=None):
    """Every draw of one row against the reference; returns the figures (a dict) and raises AssertionError on a miss.
    Exact: length-M non-decreasing list inside the scored set, no zero-weight hypothesis.  To eps: every draw's position lies in
    its hypothesis' interval, and |count_i - M p_i| < 1 + M eps."""
    idx = np.asarray(idx)
    M, N = len(idx), len(s)
    w, fin = weights(s, beta)
    if w is None:
        assert np.all(idx == -1)
        return {"eps": 0.0, "cdf_miss": 0.0, "count_miss": 0.0}
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(idx) >= 0)
    assert fin[idx].all() and np.all(w[idx] > 0)
    p, E, C = cdf(s, beta)
    eps = tolerance(s, beta)
    t = (np.arange(M, dtype=LD) + LD(offset_of(u))) / LD(M)
    miss = float(np.maximum(E[idx] - t, t - C[idx]).max())
    count = np.bincount(idx, minlength=N)
    cmiss = float(np.abs(count - M * p).max())
    fig = {"eps": eps, "cdf_miss": miss, "count_miss": cmiss}
    assert miss <= eps, fig
    assert cmiss < 1 + M * eps, fig
    return fig


def compose_rotations_indexed(idx, R, D):
    """out[b, j] = R[idx[b, j]] @ D[j] in fp32; an index outside [0, N) composes row 0.  R (N,3,3) or (B,N,3,3)."""
    idx = np.asarray(idx)
    R = np.asarray(R, dtype=np.float32)
    D = np.asarray(D, dtype=np.float32)
    N = R.shape[-3]
    loc = np.where((idx < 0) | (idx >= N), 0, idx)
    seeds = R[np.arange(len(idx))[:, None], loc] if R.ndim == 4 else R[loc]      # (B, M, 3, 3)
    return np.matmul(seeds, D[None]).astype(np.float32)
