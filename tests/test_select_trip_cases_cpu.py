"""CPU twin of tests/test_gpu_select_trips.py: what the GPU tests assume of their inputs (tests/select_trip_cases.py), asserted
with the references alone -- the decision margins of the pinned seeds, the posterior's conditioning, every plant where it is said
to be, members behind the first second-trip tile, and the walk itself for every size.  It also reads the caps from the kernel
sources: whoever changes one is told here that the sizes no longer reach a second trip."""
import numpy as np
import pytest

from . import posterior_reference as pr
from . import resample_reference as rr
from . import select_trip_cases as tc
from . import sym_reference as sr
from . import views_reference as vr

SYM_MARGIN, SYM_MAX_LEFT_OUT = 1e-5, 0.01      # test_gpu_sym.py's


# ---- the walk -----------------------------------------------------------------------------------------------------------

def test_caps_are_the_sources():
    src = tc.source_constants()
    assert src == {"kTopkThreads": tc.TOPK_THREADS, "kTopkPerLane": tc.TOPK_PER_LANE, "kTileGridMax": tc.TILE_GRID_MAX,
                   "kPostMaxParts": tc.POST_MAX_PARTS, "kTopkMaxParts": tc.TOPK_MAX_PARTS}, src
    assert tc.TILE == 1024


def in_tile(N, t):
    """Hypotheses of tile t."""
    return min(N, (t + 1) * tc.TILE) - t * tc.TILE


def test_trips_of_the_posterior_sizes():
    cap = tc.POST_MAX_PARTS
    w = tc.trips(64512, cap)
    assert len(w) == 63 and all(x == [i] for i, x in enumerate(w)) and tc.second_trip_start(64512, cap) is None   # the control
    assert in_tile(64512, 62) == 1024
    w = tc.trips(64513, cap)
    assert w[0] == [0, 63] and all(x == [i] for i, x in enumerate(w) if i) and in_tile(64513, 63) == 1
    assert tc.second_trip_start(64513, cap) == 64512
    w = tc.trips(129027, cap)
    assert w[0] == [0, 63, 126] and all(x == [i, i + 63] for i, x in enumerate(w) if i) and in_tile(129027, 126) == 3
    assert (9 * 129027) % 4 == 3 and 129027 % 4 == 3          # sample 1's rows of R and of the scores start mid-vector


def test_trips_of_the_lane_sizes():
    w = tc.trips(65537, tc.WAVE)
    assert w[0] == [0, 64] and all(x == [i] for i, x in enumerate(w) if i) and in_tile(65537, 64) == 1
    w = tc.trips(131075, tc.WAVE)
    assert w[0] == [0, 64, 128] and all(x == [i, i + 64] for i, x in enumerate(w) if i) and in_tile(131075, 128) == 3
    # the scan's boundary loop runs over tiles + 1 records
    assert tc.tiles_of(65537) + 1 == 66 and tc.tiles_of(131075) + 1 == 130


def test_trips_of_the_grid_sizes():
    cap = tc.TILE_GRID_MAX
    w = tc.trips(1048577, cap)
    assert len(w) == 1024 and w[0] == [0, 1024] and all(x == [i] for i, x in enumerate(w) if i) and in_tile(1048577, 1024) == 1
    w = tc.trips(1049603, cap)
    assert w[0] == [0, 1024] and w[1] == [1, 1025] and all(x == [i] for i, x in enumerate(w) if i > 1)
    assert in_tile(1049603, 1024) == 1024 and in_tile(1049603, 1025) == 3 and 1049603 % 4 == 3 and 1049603 == 2 ** 20 + 1027
    for N in tc.GRID_SIZES + tc.LANE_SIZES:
        assert tc.tiles_of(N) > tc.TOPK_MAX_PARTS            # (topk_kernel's walk, covered by test_gpu_topk.py, is past its cap too)


def test_tiling():
    base = np.arange(tc.BASE * 9, dtype=np.float32).reshape(tc.BASE, 3, 3)
    big = tc.tiled(base, 3 * tc.BASE + 5)
    assert big.shape == (3 * tc.BASE + 5, 3, 3) and np.array_equal(big[2 * tc.BASE + 7], base[7]) and np.array_equal(big[:tc.BASE], base)
    both = tc.tiled(np.stack([base, -base]), 5000)
    assert both.shape == (2, 5000, 3, 3) and np.array_equal(both[1, 4100], -base[1])
    assert all(tc.BASE % p for p in range(2, 65))             # prime: tile t starts at base entry (1024 t) % 4099, all distinct
    assert len({(tc.TILE * t) % tc.BASE for t in range(1026)}) == 1026


# ---- 1. modes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,per_sample", sorted(tc.MODES_CASES))
def test_modes_margin_and_plants(N, per_sample):
    s, R, plants = tc.modes_case(N, per_sample)
    want, margin = tc.modes_want(N, per_sample)
    print("modes N=%d per=%s: margin %.3e" % (N, per_sample, margin))
    assert margin >= tc.MARGIN
    start = tc.second_trip_start(N, tc.TILE_GRID_MAX)
    assert plants["a"][1] == N - 1 >= start and s[0].max() == s[0, N - 1] == tc.TOP
    tc.check_modes_plants(want, plants)
    assert np.sort(s[0])[-2] < tc.FOURTH or "b" in plants       # the plants are above every drawn score
    if "b" in plants:
        assert N == 1049603
        Rb = lambda b: R[b] if per_sample else R
        (_, ia), (_, ib) = plants["a"], plants["b"]
        assert np.array_equal(Rb(0)[ia], Rb(0)[ib]) and np.sort(s[0])[-2] == s[0, ib] == tc.NEXT
        assert ib // tc.TILE == 1020                            # a first-trip tile: the kill crosses the trips
        (_, ic), (_, jc), (_, ie), (_, jd) = plants["c"], plants["c_copy"], plants["e"], plants["d"]
        assert ic < start and ie < start and jc // tc.TILE == jd // tc.TILE == 1025 and np.array_equal(Rb(1)[ic], Rb(1)[jc])
        top4 = np.argsort(-s[1], kind="stable")[:4]
        assert top4.tolist() == [ic, jc, ie, jd]
        # d is outside tau of both earlier winners (it is listed third: check_modes_plants), by a margin of its own
        tau = float(tc.mr.tau_of(tc.MODES_ANGLE))
        for w in (ic, ie):
            assert float(np.sum(Rb(1)[jd].astype(np.float64) * Rb(1)[w].astype(np.float64))) < tau - tc.MARGIN


# ---- 2. modes modulo a group, and the fold ------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,per_sample", tc.SYM_MODES_CASES)
def test_sym_margin_and_plants(group, per_sample):
    s, R, sym, plants = tc.sym_case(group, per_sample)
    S, axis = tc.sym_np(sym)
    want, margin = tc.sym_want(group, per_sample)
    print("sym modes %s per=%s: margin %.3e" % (group, per_sample, margin))
    assert margin > SYM_MARGIN
    tc.check_modes_plants(want, plants, tc.SYM_OFFSET)
    tau = sr.tau_of(tc.SYM_ANGLE)
    for copy, of in (("b", "a"), ("c_copy", "c")):
        (b, i), (_, w) = plants[copy], plants[of]
        Rb = R[b] if per_sample else R
        plain = float(np.sum(Rb[i].astype(np.float64) * Rb[w].astype(np.float64)))
        t_g = float(sr.sym_trace(Rb[i][None], Rb[w], S, axis)[0][0])
        assert plain < tau - 1.0 and t_g > 3.0 - 1e-5          # far from the winner as a rotation, the same pose modulo the group


@pytest.mark.parametrize("group", sorted(tc.SYM_GROUPS))
def test_fold_left_out_share(group):
    """test_gpu_sym.py's cap on the decisions left out (margin 1e-5), met by the base set on its own and by the kept run."""
    R, sym, anchors, V = tc.fold_case(group)
    S, axis = tc.sym_np(sym)
    base = sr.fold(R[:, :tc.BASE], S, axis, anchors, tc.FOLD_ANGLE, 0, V[:, :tc.BASE])
    assert 1.0 - (base["margin"] > SYM_MARGIN).mean() <= SYM_MAX_LEFT_OUT
    assert sorted(np.unique(base["which"]).tolist()) == [-1, 0, 2]                 # slot 1 is empty; both others take something
    assert tc.second_trip_start(tc.SYM_N, tc.TILE_GRID_MAX) < tc.FOLD_KEEP < tc.SYM_N and tc.FOLD_KEEP % 4 != 0
    kept = sr.fold(R, S, axis, anchors, tc.FOLD_ANGLE, tc.FOLD_KEEP, V)
    assert 1.0 - (kept["margin"] > SYM_MARGIN).mean() <= SYM_MAX_LEFT_OUT
    assert np.all(kept["which"][:, :tc.FOLD_KEEP] == -1)
    for k in (0, 2):                                                               # both anchors and several elements behind keep
        assert (kept["which"][:, tc.FOLD_KEEP:] == k).sum(axis=1).min() >= 10
    assert len(np.unique(kept["elem"][kept["which"] >= 0])) == (4 if group == "d2" else 1) and kept["moved"].any()


# ---- 3. posterior -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,per_sample", sorted(tc.POST_CASES))
def test_posterior_margin_conditioning_and_members(N, per_sample):
    s, R, A = tc.posterior_case(N, per_sample)
    assert s.shape == (tc.POST_B, N) and np.isfinite(s).all() and np.all(np.any(A != 0, axis=(2, 3)))   # four live anchors
    for temp in tc.POST_TEMPS:
        want, margin = tc.posterior_want(N, per_sample, temp)
        cond = want["cond"][:, :tc.POST_K]
        print("posterior N=%d per=%s T=%g: margin %.3e, min mode cond %.3f" % (N, per_sample, temp, margin, np.nanmin(cond)))
        assert margin >= tc.MARGIN and not np.isnan(cond).any() and np.all(cond >= tc.MIN_COND)
    bucket = tc.posterior_buckets(N, per_sample)
    start = tc.second_trip_start(N, tc.POST_MAX_PARTS)
    if N == 64512:
        assert start is None
    elif N == 64513:
        assert start == N - 1            # ONE hypothesis: it is in one bucket; the membership counts of the GPU test see it
    else:
        third = 2 * tc.POST_MAX_PARTS * tc.TILE
        for b in range(tc.POST_B):       # every bucket, the rest included, has members in second-trip tiles; the three
            assert set(bucket[b, start:third].tolist()) == set(range(tc.POST_K + 1))   # third-trip hypotheses are counted
        assert N - third == 3


def test_posterior_holes_sit_in_the_stated_trips():
    N = 129027
    w = tc.trips(N, tc.POST_MAX_PARTS)
    trip_of = {t: k for x in w for k, t in enumerate(x)}
    seen = set()
    for b, t, place, _ in tc.POST_HOLES:
        assert t * tc.TILE + place < N and b in (0, 2)             # sample 1 is the all-NaN one
        seen.add(trip_of[t])
    assert seen == {0, 1, 2}
    assert len({(b, t, p) for b, t, p, _ in tc.POST_HOLES}) == len(tc.POST_HOLES)


def test_posterior_stock_figures():
    """The yardstick of the GPU test's bars: the stock fp32 composition against fp64 over exactly POST_CASES.  The recorded
    figures are those of this measurement (a thread count or a BLAS moves an fp32 sum: a factor 2 either way is allowed)."""
    worst = {k: 0.0 for k in tc.POST_STOCK_ERR}
    for (N, per_sample) in sorted(tc.POST_CASES):
        s, R, A = tc.posterior_case(N, per_sample)
        for temp in tc.POST_TEMPS:
            want, _ = tc.posterior_want(N, per_sample, temp)
            e = pr.errors(pr.stock_fp32(s, R, A, tc.POST_ANGLE, temp), want, want["cond"], tc.MIN_COND)
            worst = {k: max(worst[k], e[k]) for k in worst}
    print("stock fp32 over the trip cases:", worst)
    for k, v in tc.POST_STOCK_ERR.items():
        assert 0.5 * v <= worst[k] <= 2.0 * v, (k, worst[k], v)


# ---- 4. resample --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", tc.RES_SIZES)
def test_resample_rows(N):
    tiles = tc.tiles_of(N)
    assert tiles > tc.WAVE and (N in tc.LANE_SIZES or tiles > tc.TILE_GRID_MAX)
    s = tc.resample_last_tile_rows(N)
    fin = np.isfinite(s)
    assert fin[:, (tiles - 1) * tc.TILE:].all() and not fin[:, :(tiles - 1) * tc.TILE].any() and tiles - 1 >= 64
    s = tc.resample_equal_rows(N)
    assert np.isfinite(s[0]).all() and (~np.isfinite(s[1])).sum() == 3 and not np.isfinite(s[1, N - 1])   # a hole in the last tile
    s = tc.resample_random_rows(N)
    assert all((~np.isfinite(s[b])).sum() == 3 for b in range(tc.RES_B))
    # the reference's own consistency on a row of this size: the draws by the definition = the draws by boundaries
    a = rr.resample_row(s[0], rr.beta_of(0.1), 5000, 0.5)
    assert np.array_equal(a, rr.resample_row_by_boundaries(s[0], rr.beta_of(0.1), 5000, 0.5))
    assert a.max() >= (tc.WAVE if N in tc.LANE_SIZES else tc.TILE_GRID_MAX) * tc.TILE - tc.TILE   # draws reach the last tiles


# ---- 5. views -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_sample", [True, False])
@pytest.mark.parametrize("N", tc.VIEWS_SIZES)
def test_views_margin_members_and_plant(N, per_sample):
    s, Q, A = tc.views_case(N, per_sample)
    slot, counts, g, margin = tc.views_compact_want(N, per_sample)
    print("views N=%d per=%s: margin %.3e, counts %s" % (N, per_sample, margin, counts.tolist()))
    assert margin >= tc.MARGIN
    assert not counts[:, 1].any() and np.all(counts[:, [0, 2]] > 0) and counts.sum() < 0.2 * g.size   # the limit decides
    start = tc.second_trip_start(N, tc.WAVE if N in tc.LANE_SIZES else tc.TILE_GRID_MAX)
    behind = g[:, :, start:].sum(axis=2)
    assert np.all(g[:, 0, N - 1])                        # view 0 takes part in the planted hypothesis, the last one
    if N - start > 1:                                    # (a second trip of ONE hypothesis cannot serve both live views)
        assert np.all(behind[:, [0, 2]] > 0)
    for theta in (None, tc.VIEWS_THETA):                 # the plant is the fused row's arg-max, with and without the limit
        S, scale, _, _ = vr.fuse(s, Q, A, tc.VIEWS_WEIGHTS, theta)
        assert not np.isnan(S).any() and not np.isposinf(S).any()
        score, idx = vr.decode(vr.best_keys(S, tc.VIEWS_OFFSET))
        assert idx.tolist() == [N - 1 + tc.VIEWS_OFFSET] * tc.VIEWS_B and score.tolist() == [tc.VIEWS_BEST] * tc.VIEWS_B
