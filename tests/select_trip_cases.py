"""Inputs of the second-trip tests of the selection kernels (tests/test_gpu_select_trips.py) and of their CPU twin
(tests/test_select_trip_cases_cpu.py).  Plain module (like tests/modes_reference.py): numpy and the references, no GPU.

The selection family (ahv_select.hip, ahv_views.hip, ahv_posterior.hip; grid rule: ahv_tile.h) cuts a sample's N hypotheses into
tiles of 1024 and caps the workgroups per sample; past the cap workgroup x walks the tiles x, x + cap, ...  ``trips`` restates
that walk and the sizes below are named for what they reach.  The same pattern inside one wave (``for (i = lane; i < tiles; i +=
64)``) is the cap 64.

Every test of the family first asserts the reference's decision margin (the smallest |t - tau| met in fp64).  With N independent
Haar rotations that margin shrinks like 1 / N and no seed holds 1e-4 at 10^5 .. 10^6 hypotheses, so the large sets here are a
small Haar base set repeated cyclically, ``R_big[n] = R_base[n % 4099]``: 4099 is prime, so every tile sees a different stretch
of the base; the set of distinct t values is the base set's, so the margin is that of an N = 4099 case; a copy of a winner has
t = 3, far above any tau.  Scores are drawn per hypothesis, not repeated.  The seeds are pinned by the CPU twin.
"""
import importlib
import os
import re

import numpy as np

from . import modes_reference as mr
from . import posterior_reference as pr
from . import sym_reference as sr
from . import views_compact_reference as vcr
from . import views_reference as vr

# ---- the walk -----------------------------------------------------------------------------------------------------------
# copies of the sources' constants (the CPU twin compares them with ahv_tile.h, ahv_posterior.hip and ahv_select.hip)
TOPK_THREADS, TOPK_PER_LANE, TILE_GRID_MAX, POST_MAX_PARTS, TOPK_MAX_PARTS = 256, 4, 1024, 63, 63
TILE = TOPK_THREADS * TOPK_PER_LANE
WAVE = 64
BASE = 4099

POST_SIZES = (64512, 64513, 129027)   # cap 63: 63 full tiles (the control), one hypothesis in a second trip, a third trip
LANE_SIZES = (65537, 131075)          # 64 lanes: lane 0 takes a second record / tile count, lanes 0 and 1 take a third
GRID_SIZES = (1048577, 1049603)       # cap 1024: one hypothesis in a second trip; a full tile and three ragged hypotheses

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dahv_amd", "csrc")


def source_constants():
    """The caps as the sources state them: {name: int}."""
    out = {}
    for fname, names in (("ahv_tile.h", ("kTopkThreads", "kTopkPerLane", "kTileGridMax")), ("ahv_posterior.hip", ("kPostMaxParts",)),
                         ("ahv_select.hip", ("kTopkMaxParts",))):
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for name in names:
            m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
            assert m, (fname, name)
            out[name] = int(m.group(1))
    return out


def tiles_of(N):
    return (N + TILE - 1) // TILE


def trips(N, cap):
    """The tiles each workgroup (cap 63, 1024) or lane (cap 64) takes, in order: a list of min(tiles, cap) lists."""
    tiles = tiles_of(N)
    groups = min(tiles, cap)
    return [list(range(x, tiles, groups)) for x in range(groups)]


def second_trip_start(N, cap):
    """The first hypothesis that lies in a second-trip tile, None when no workgroup takes one."""
    return cap * TILE if tiles_of(N) > cap else None


def tiled(base, N, axis=-3):
    """``base`` repeated cyclically along ``axis`` (the hypothesis axis: -3 for matrices (..., n, 3, 3)) to length N."""
    base = np.asarray(base)
    return np.ascontiguousarray(np.take(base, np.arange(N) % base.shape[axis], axis=axis))


def _haar(n, seed):
    return importlib.import_module("3dahv_amd").rotations.haar_rotations_np(n, seed)


_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- 1. modes -------------------------------------------------------------------------------------------------------------
MODES_K, MODES_ANGLE, MODES_OFFSET, MODES_B = 8, 15.0, 7, 2
# (N, per-sample R) -> seed
MODES_CASES = {(1048577, True): 0, (1049603, True): 0, (1049603, False): 0}
TOP, NEXT, THIRD, FOURTH = 8.0, 7.0, 6.5, 6.0   # above every N(0,1) draw of 2 x 10^6 (the largest is about 5.2)


def modes_plants(N):
    """{name: (sample, index)} -- what each is for: the docstring of test_gpu_select_trips.py.
    a: the row's largest score at N - 1 (a second-trip tile); b: the next-largest one period earlier, the same matrix (at
    1 049 603 the second trip holds 1027 hypotheses, fewer than a period: b lies in tile 1020, so the kill of a second-trip winner
    has to reach a first-trip tile).  c: sample 1's largest in the first trip; c_copy: the same matrix in the last tile with the
    next-largest score; e: the third-largest, first trip; d: the fourth-largest in the last tile."""
    plants = {"a": (0, N - 1)}
    if N - 1 - BASE >= 0 and N > TILE_GRID_MAX * TILE + 1:
        last = (tiles_of(N) - 1) * TILE
        plants.update(b=(0, N - 1 - BASE), c=(1, last - 100 * BASE), c_copy=(1, last), e=(1, 12345), d=(1, last + 1))
    return plants


PLANT_SCORE = {"a": TOP, "b": NEXT, "c": TOP, "c_copy": NEXT, "e": THIRD, "d": FOURTH}


def modes_case(N, per_sample):
    """(scores (B,N), R (B,N,3,3) or (N,3,3), plants) of a case, made once and never modified."""
    def make():
        seed = MODES_CASES[(N, per_sample)]
        s = np.random.default_rng(seed).standard_normal((MODES_B, N)).astype(np.float32)
        base = _haar(BASE * (MODES_B if per_sample else 1), seed + 1)
        R = tiled(base.reshape(MODES_B, BASE, 3, 3) if per_sample else base, N)
        plants = modes_plants(N)
        for name, (b, i) in plants.items():
            s[b, i] = PLANT_SCORE[name]
        return s, R, plants
    return _once(("modes", N, per_sample), make)


def modes_want(N, per_sample):
    """(keys (B,K) int64, margin) of ``modes_reference.select_modes`` on the case, computed once."""
    def make():
        s, R, _ = modes_case(N, per_sample)
        return mr.select_modes(s, R, MODES_K, MODES_ANGLE, n_offset=MODES_OFFSET)
    return _once(("modes_want", N, per_sample), make)


def check_modes_plants(keys, plants, n_offset=MODES_OFFSET):
    """Asserts on a (B,K) key list what the plants are there for."""
    idx = mr.indices(np.asarray(keys)) - n_offset
    assert idx[0, 0] == plants["a"][1]
    if "b" in plants:
        assert plants["b"][1] not in idx[0].tolist()
        assert idx[1, 0] == plants["c"][1] and plants["c_copy"][1] not in idx[1].tolist()
        assert idx[1, 1] == plants["e"][1] and idx[1, 2] == plants["d"][1]


# ---- 2. modes modulo a group, and the fold --------------------------------------------------------------------------------
SYM_N, SYM_B, SYM_K, SYM_ANGLE, SYM_OFFSET = 1049603, 2, 4, 15.0, 7
SYM_GROUPS = {"d2": 1, "cinf": 2}     # group -> seed (per-sample R: the mode lists and the folds)
SYM_SHARED = {"cinf": 0}              # group -> seed of the one mode list over a shared R
SYM_MODES_CASES = [(g, True) for g in sorted(SYM_GROUPS)] + [(g, False) for g in sorted(SYM_SHARED)]
FOLD_K, FOLD_ANGLE = 3, 60.0
FOLD_KEEP = TILE_GRID_MAX * TILE + 501    # inside tile 1024, the first tile of a second trip, and off the lanes' grid of four


def _group(name):
    Sy = importlib.import_module("3dahv_amd").rotations.Symmetry
    return {"d2": lambda: Sy.dihedral(2, (1.0, 2.0, 2.0)), "cinf": lambda: Sy.axial((2.0, -1.0, 2.0))}[name]()


def _axis_turn(axis, deg):
    return sr.rot(np.asarray(axis, np.float64), np.array([np.cos(np.radians(deg))]), np.array([np.sin(np.radians(deg))]))[0]


def sym_case(group, per_sample=True):
    """(scores (B,N), R (B,N,3,3) or (N,3,3), sym, plants): ``modes_case`` at 1 049 603, where the copies b and c_copy are ORBIT
    MEMBERS of their winners instead (R_w S_1 for d2, R_w Rot(axis, 100 degrees) for the axial group): 100 degrees or more from
    the winner as plain rotations, the same pose modulo the group.  (A shared R holds both samples' members; the other sample
    sees each under a drawn score.)"""
    def make():
        seed = (SYM_GROUPS if per_sample else SYM_SHARED)[group]
        N = SYM_N
        sym = _group(group)
        s = np.random.default_rng(seed + 10).standard_normal((SYM_B, N)).astype(np.float32)
        base = _haar(BASE * (SYM_B if per_sample else 1), seed + 11)
        R = tiled(base.reshape(SYM_B, BASE, 3, 3) if per_sample else base, N)
        plants = modes_plants(N)
        for name, (b, i) in plants.items():
            s[b, i] = PLANT_SCORE[name]
        member = sym.S[1].numpy().astype(np.float64) if sym.axis is None else _axis_turn(sym.axis.numpy(), 100.0)
        for copy, of in (("b", "a"), ("c_copy", "c")):
            (b, i), (_, w) = plants[copy], plants[of]
            Rb = R[b] if per_sample else R
            Rb[i] = (Rb[w].astype(np.float64) @ member).astype(np.float32)
        return s, R, sym, plants
    return _once(("sym", group, per_sample), make)


def sym_np(sym):
    return sym.S.numpy(), (None if sym.axis is None else sym.axis.numpy())


def sym_want(group, per_sample=True):
    def make():
        s, R, sym, _ = sym_case(group, per_sample)
        return sr.select_modes(s, R, SYM_K, SYM_ANGLE, *sym_np(sym), n_offset=SYM_OFFSET)
    return _once(("sym_want", group, per_sample), make)


def fold_case(group):
    """(R (B,N,3,3), sym, anchors (B,3,3,3) with slot 1 empty, V (B,N,3)) on the rotations of ``sym_case``."""
    def make():
        _, R, sym, _ = sym_case(group)
        seed = SYM_GROUPS[group]
        anchors = _haar(SYM_B * FOLD_K, seed + 12).reshape(SYM_B, FOLD_K, 3, 3).copy()
        anchors[:, 1] = 0.0
        V = (np.random.default_rng(seed + 13).standard_normal((SYM_B, SYM_N, 3)) * 0.1).astype(np.float32)
        return R, sym, anchors, V
    return _once(("fold", group), make)


# ---- 3. posterior -----------------------------------------------------------------------------------------------------------
POST_K, POST_ANGLE, POST_B, POST_TEMPS = 4, 30.0, 3, (0.1, 0.02)
POST_NOISE = 0.02
MARGIN, MIN_COND = 1e-4, 0.5          # test_gpu_posterior.py's
# the error of the stock fp32 torch composition (posterior_reference.stock_fp32) against the fp64 reference over exactly
# POST_CASES at both temperatures, measured on the CPU: scalars, mean rotations (degrees), spreads (degrees).  The CPU twin
# measures them again; test_gpu_select_trips.py holds the kernels to 4 x these (test_gpu_posterior.py's rule).
POST_STOCK_ERR = {"scalar": 4.3e-7, "rot_deg": 0.0494, "spread_deg": 1.17e-3}
# (N, per-sample R) -> seed of posterior_reference.make_inputs(4099, 3, per, seed)
POST_CASES = {(64512, True): 1, (64513, True): 1, (129027, True): 1, (129027, False): 0}


def posterior_case(N, per_sample):
    """(scores (B,N), R, anchors (B,K,3,3)): base set, its planted-peak scores and its modes as anchors from
    ``posterior_reference.make_inputs`` at 4099; R tiled; the scores tiled (they are a function of the matrix) plus N(0, 0.02^2)
    noise drawn per hypothesis, so that no two tiles hold the same scores."""
    def make():
        seed = POST_CASES[(N, per_sample)]
        s0, R0, A = _once(("post_base", per_sample, seed),
                          lambda: pr.make_inputs(BASE, POST_B, per_sample, seed, K=POST_K, angle_deg=POST_ANGLE))
        noise = np.random.default_rng(seed + 1000).standard_normal((POST_B, N)).astype(np.float32) * np.float32(POST_NOISE)
        return (tiled(s0, N, axis=-1) + noise).astype(np.float32), tiled(R0, N), A
    return _once(("post", N, per_sample), make)


def posterior_want(N, per_sample, temp):
    def make():
        s, R, A = posterior_case(N, per_sample)
        return pr.posterior(s, R, A, POST_ANGLE, temp)
    return _once(("post_want", N, per_sample, temp), make)


def posterior_buckets(N, per_sample):
    """(B,N) bucket of every hypothesis (K = the rest) by the reference's rule."""
    def make():
        _, R, A = posterior_case(N, per_sample)
        tau = pr.tau_of(POST_ANGLE)
        return np.stack([pr.assign(R[b] if per_sample else R, A[b], tau)[0] for b in range(POST_B)])
    return _once(("post_buckets", N, per_sample), make)


# where the non-finite scores of the exclusion test go at 129 027: (sample, tile, place in the tile, value); tiles 0 and 62 are a
# workgroup's first trip, 63 and 125 its second, 126 (workgroup 0, ragged: three hypotheses) its third
POST_HOLES = [(0, 0, 5, np.nan), (0, 63, 1023, np.inf), (0, 126, 2, -np.inf), (0, 125, 0, np.nan),
              (2, 62, 17, np.inf), (2, 64, 512, np.nan), (2, 126, 0, np.nan)]


# ---- 4. resample --------------------------------------------------------------------------------------------------------------
RES_B = 2
RES_SIZES = LANE_SIZES + GRID_SIZES
RES_US = [0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), 1.5, float("nan")]   # test_gpu_resample.py's US


def resample_holes(s):
    """NaN / +inf / -inf holes, a different place in every row, one of them in the last tile."""
    N = s.shape[1]
    for b in range(s.shape[0]):
        s[b, (b + 1) % N], s[b, (N // 2 + b) % N], s[b, N - 1 - b % 2] = np.nan, np.inf, -np.inf
    return s


def resample_equal_rows(N):
    """Rows of equal scores (weights of exactly 1): row 0 whole, row 1 with holes."""
    s = np.full((RES_B, N), 0.25, np.float32)
    s[1] = -0.75
    s[1:] = resample_holes(s[1:])
    return s


def resample_random_rows(N):
    return resample_holes(np.random.default_rng(1000 + N).uniform(-0.2, 0.6, (RES_B, N)).astype(np.float32))


def resample_last_tile_rows(N):
    """Weight in the last tile only (-inf / NaN everywhere else): the scan's ``last_tile`` is the last record."""
    s = np.full((RES_B, N), -np.inf, np.float32)
    s[1] = np.nan
    s[:, (tiles_of(N) - 1) * TILE:] = 0.5
    return s


# ---- 5. views -------------------------------------------------------------------------------------------------------------
VIEWS_B, VIEWS_V, VIEWS_THETA, VIEWS_OFFSET = 2, 3, 60.0, 3
VIEWS_WEIGHTS = [0.5, 0.0, 1.0]       # test_gpu_views.weights_for(3): the middle view is absent
VIEWS_SEEDS = {True: 0, False: 0}     # per-sample Q -> seed
VIEWS_SIZES = LANE_SIZES + GRID_SIZES
VIEWS_BEST = 50.0


def clear_of_threshold(Q, A, spare, theta=VIEWS_THETA, guard=2e-4):
    """test_gpu_views.clear_of_threshold: every hypothesis of Q (B,n,3,3) whose t to some view of its sample lies within ``guard``
    of tau is replaced, in order, by the next rotation of ``spare`` that is clear of tau for all of that sample's views."""
    tau = float(vr.tau_of(theta))
    Q = Q.copy()
    nxt = 0
    for b in range(Q.shape[0]):
        Ab = A[b].astype(np.float64)
        t = np.einsum("nij,vij->vn", Q[b].astype(np.float64), Ab)
        for n in np.flatnonzero((np.abs(t - tau) < guard).any(axis=0)):
            while True:
                c = spare[nxt]
                nxt += 1
                if (np.abs(np.einsum("ij,vij->v", c.astype(np.float64), Ab) - tau) >= guard).all():
                    Q[b, n] = c
                    break
    return Q


def views_base(per_sample):
    """(Q base (B,4099,3,3) or (4099,3,3), A (B,V,3,3)): Haar, kept clear of the 60-degree threshold (for a shared Q: of every
    sample's views).  The base entries that land on hypothesis N - 1 of each size are view 0's own pose (t = 3: view 0 takes
    part there whatever the limit), which is where the best score is planted; a shared Q gives every sample the same view 0."""
    def make():
        seed = VIEWS_SEEDS[per_sample]
        A = _haar(VIEWS_B * VIEWS_V, seed + 21).reshape(VIEWS_B, VIEWS_V, 3, 3).copy()
        if not per_sample:
            A[:, 0] = A[0, 0]
        nb = VIEWS_B if per_sample else 1
        pool = _haar(nb * BASE + 1024, seed + 20)
        raw, spare = pool[:nb * BASE].reshape(nb, BASE, 3, 3), pool[nb * BASE:]
        Q = clear_of_threshold(raw, A if per_sample else A.reshape(1, VIEWS_B * VIEWS_V, 3, 3), spare)
        for N in VIEWS_SIZES:
            Q[:, (N - 1) % BASE] = A[:nb, 0]
        return (Q if per_sample else Q[0]), A
    return _once(("views_base", per_sample), make)


def views_case(N, per_sample):
    """(scores (B,V,N), Q, A): N(0,1) scores per pair, the absent view's row all NaN (it is never read), a -inf in each live row,
    and VIEWS_BEST for both live views at hypothesis N - 1, a second-trip tile: the fused row's largest value."""
    def make():
        Qb, A = views_base(per_sample)
        rng = np.random.default_rng(VIEWS_SEEDS[per_sample] + N)
        s = rng.standard_normal((VIEWS_B, VIEWS_V, N)).astype(np.float32)
        s[:, 1] = np.nan
        for b in range(VIEWS_B):
            for v in (0, 2):
                s[b, v, rng.integers(0, N - 1)] = -np.inf
                s[b, v, N - 1] = VIEWS_BEST
        return s, tiled(Qb, N), A
    return _once(("views", N, per_sample), make)


def views_compact_want(N, per_sample):
    """(slot (B,V,N) int32, counts (B,V), g, margin) of ``views_compact_reference.compact`` on the case, computed once."""
    def make():
        _, Q, A = views_case(N, per_sample)
        return vcr.compact(Q, A, VIEWS_THETA, VIEWS_WEIGHTS)
    return _once(("views_compact", N, per_sample), make)
