"""The host mirror of the device's random streams (tests/rng_reference.py), the partition of the Philox counter space, and the
conditions of the cases tests/test_gpu_rng.py runs -- no GPU.

What it holds in place:
  * the mirror's Philox-4x32-10 against the three Random123 known-answer vectors, and its fp64 composition against Rodrigues'
    formula written independently;
  * the tags and fresh-slot seeds of ahv_so3.h, ahv_track.hip and ahv_graph.hip against the values include/ahv.h states, and the
    C expressions those files build their counters, keys and fresh offsets from -- read from the sources and evaluated with C's
    unsigned widths -- against the mirror's layouts, which are written from the header's wording.  Editing a tag, a bit field
    or an offset formula in a source fails here;
  * the partition, by arithmetic: the low 24 bits of the third counter word differ between every pair of the five streams; each
    stream's (key, counter) has a left inverse over the ranges the header allows (so the map is injective there), every bit of
    every argument inside its range changes the tuple, and the bits the header says are dropped -- step[63:48] of the tracker's
    noise, t[63:40] of the pose graph's -- do not; ahv_track_advance takes all 64 bits of its counter;
  * the two fresh-slot offset formulas: mixed-radix numbers, injective while they stay below 2^64, which is
    (step + 1) B M <= 2^64 for the tracker and (t + 1) 2^28 N <= 2^64 for the pose graph; past that they wrap, as the header says;
  * the one known overlap: tracker and pose graph draw their fresh slots from the SAME Haar stream (seed ^ 0x9E3779B97F4A7C15), so
    with equal seeds tracker step 1, B = 1, M = 512 and graph t = 0, sweep 0, b = 0, k = 1, N = 512 both hold offsets 512..1023.
    Recorded as it is; the header makes distinct seeds a condition on the caller.

Figures (printed by a run with -s):
  source expressions against the mirror at 718 argument tuples x 8 layouts; 10 pairs of tags
  left inverse at 1 225 (haar), 4 096 (diffuse, velocity), 2 523 (advance), 2 410 (graph) argument tuples; bits that change the
  tuple / bits the header drops: haar 128 / 0, diffuse and velocity 159 / 16, advance 144 / 0, graph 163 / 24
  fresh offsets: 120 argument tuples recovered by divmod
  edge blocks of seed 0x3DA4F: radius_zero at 29 601 500, radius_max at 5 596 761, angle_zero at 19 999 506
"""
import itertools
import os
import re

import numpy as np
import pytest

from . import rng_cases as rc
from . import rng_reference as rr

HEADER = os.path.join(rr.REPO, "include", "ahv.h")
M32, M64 = rr.M32, rr.M64


def _tuple(block):
    return tuple(int(np.asarray(x).reshape(-1)[0]) for x in block)


# ---- 1. the algorithm ---------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(x) for x in rr.philox4x32_10(*ctr, *key)) == want
    # vectorised: the three at once, and neither nine rounds nor swapped key words give these
    c = [np.array([k[0][w] for k in KAT]) for w in range(4)]
    k = [np.array([k[1][w] for k in KAT]) for w in range(2)]
    got = np.stack(rr.philox4x32_10(*c, *k), axis=-1)
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))
    assert not np.array_equal(np.stack(rr.philox4x32(*c, *k, rounds=9), axis=-1)[0], got[0])
    assert not np.array_equal(np.stack(rr.philox4x32_10(*c, k[1], k[0]), axis=-1)[2], got[2])


def _rodrigues(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if a < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * (K @ K)


def test_mirror_composition_is_r_times_exp():
    """The fp64 mirror against R exp([w]x) by Rodrigues' formula, over every Shepperd branch and both sides of the small-angle
    switch; the fp32 mirror stays within a few ulp of it."""
    R32, br = rc.pool()
    rs = np.random.RandomState(5)
    worst = worst32 = 0.0
    for branch in range(4):
        for k in range(3):
            R = rc.of_branch(branch, k)
            for scale in (0.0, 1e-6, 9.99e-4, 1.01e-3, 0.05, 1.0, 3.0):
                w = (scale * rs.standard_normal(3) / np.sqrt(3)).astype(np.float32)
                want = R.astype(np.float64) @ _rodrigues(w.astype(np.float64))
                got = rr.compose_rotation_vector(R[None], w[None], np.float64)[0]
                got32 = rr.compose_rotation_vector(R[None], w[None], np.float32)[0]
                assert got32.dtype == np.float32
                worst = max(worst, float(np.abs(got - want).max()))
                worst32 = max(worst32, float(np.abs(got32 - want).max()))
    print("mirror composition against Rodrigues: fp64 %.2e, fp32 %.2e" % (worst, worst32))
    # R is an fp32 rotation: orthonormal to ~1e-7 only, and the mirror normalises where Rodrigues does not
    assert worst <= 1e-6 and worst32 <= 2e-6
    assert set(br.tolist()) == {0, 1, 2, 3}


def test_mirror_haar_rotations_are_rotations():
    R = rr.haar_rotation(3, np.arange(2000))
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(R) - 1).max() < 1e-14
    g = np.stack(rr.box_muller4(rr.draw(rr.haar_block(3, np.arange(20000)))), axis=-1)
    assert abs(g.mean()) < 0.02 and abs(g.std() - 1) < 0.02                     # the mirror itself is a normal sampler
    assert np.abs(np.corrcoef(g.T) - np.eye(4)).max() < 0.03
    # clip_norm: the bound holds with room, and vectors inside the limit are untouched
    w = np.random.RandomState(0).standard_normal((1000, 3))
    out, clipped = rr.clip_norm(w, 1.5)
    assert (np.linalg.norm(out, axis=-1) <= 1.5).all() and np.array_equal(out[~clipped], w[~clipped]) and rc._two_sided(clipped)
    assert np.allclose(np.linalg.norm(out[clipped], axis=-1), 1.5 * rr.CLIP_DOWN, rtol=1e-12)
    assert (rr.CLIP_UP, rr.CLIP_DOWN) == (1 + 2.0 ** -21, 1 - 2.0 ** -21)


# ---- 2. sources against the header's values -------------------------------------------------------------------------------------
def test_source_constants_are_the_headers():
    k = rr.source_constants()
    assert k == {"kHaarTag": rr.HAAR_TAG, "kDiffuseTag": rr.DIFFUSE_TAG, "kAdvanceTag": rr.ADVANCE_TAG, "kVelocityTag": rr.VELOCITY_TAG,
                 "kGraphTag": rr.GRAPH_TAG, "kFreshSeed": rr.FRESH_XOR, "kGraphFreshSeed": rr.FRESH_XOR}
    text = open(HEADER).read()
    flat = " ".join(re.sub(r"^\s*\*", " ", line) for line in text.splitlines())
    flat = " ".join(flat.split())
    for phrase in ("counter = (j, b | step[47:32] << 16, 0x444946, step[31:0])",
                   "counter = (b, (t + 1)[63:32], 0x414456, (t + 1)[31:0])",
                   "whose third counter word is 0x56454C",
                   "counter = (n, b | sweep << 16 | t[39:32] << 24, 0x504752 | k << 24, t[31:0])",
                   "counter = ((offset + n)[31:0], (offset + n)[63:32], 0x3D4148, 0)",
                   "seed ^ 0x9E3779B97F4A7C15 and offset (step * B + b) * M + j",
                   "seed ^ 0x9E3779B97F4A7C15 and offset (((t 256 + sweep) 65536 + b) 16 + k) N + n (modulo 2^64)",
                   "give the tracker and the pose graph different seeds"):
        assert phrase in flat, "include/ahv.h no longer says: " + phrase


def _env(consts, **kw):
    env = dict(consts)
    env.update({k: (v, 32) for k, v in consts.items() if "Tag" in k})
    env.update(kw)
    return env


def _source_counter(L, name, consts, **kw):
    return tuple(rr.c_eval(e, _env(consts, **kw)) for e in L[name]["counter"])


# argument tuples: every field at its ends, single bits, and random values
def _probe_values(bits, rs, n_random):
    top = (1 << bits) - 1
    return sorted({0, 1, top, top - 1, 1 << (bits - 1)} | {int(rs.randint(0, 2 ** 31)) * int(rs.randint(0, 2 ** 31)) % (top + 1)
                                                          for _ in range(n_random)})


def test_source_layouts_are_the_mirrors():
    """The kernels' counter, key and offset expressions, evaluated as C evaluates them, equal the mirror's layouts."""
    L, K = rr.source_layouts(), rr.source_constants()
    assert L["keys"] == ["(unsigned)seed, (unsigned)(seed >> 32)"] * 6          # every Philox call: key = (seed low, seed high)
    assert L["tracker_fresh"] == L["predict_fresh"] and L["tracker_fresh"]["xor"] == "kFreshSeed"
    assert L["graph_fresh"]["xor"] == "kGraphFreshSeed"
    assert L["velocity"]["counter"][2] == "kVelocityTag" and L["predict_diffuse"]["counter"][2] == "kDiffuseTag"
    rs = np.random.RandomState(11)
    n = 0
    for seed, step in itertools.product(_probe_values(64, rs, 3), _probe_values(64, rs, 8)):
        key = (rr.c_eval("(unsigned)seed", {"seed": seed}), rr.c_eval("(unsigned)(seed >> 32)", {"seed": seed}))
        for b, j, sweep, k in zip(_probe_values(16, rs, 2), _probe_values(31, rs, 2), _probe_values(8, rs, 2), (0, 15, 7, 1, 8, 3, 12)):
            b = max(b, 0)
            M, N, B = j + 1 + (step & 0xFF), j + 1 + (seed & 0xFF), min(b + 1 + (step & 3), 65535)
            assert _tuple(rr.diffuse_block(seed, step, b, j)) == key + _source_counter(L, "diffuse", K, j=j, b=b, t=step)
            assert _tuple(rr.diffuse_block(seed, step, b, j)) == key + _source_counter(L, "predict_diffuse", K, j=j, b=b, t=step)
            assert _tuple(rr.velocity_block(seed, step, b, j)) == key + _source_counter(L, "velocity", K, j=j, b=b, t=step)
            t1 = rr.c_eval(L["advance"]["t1"].replace("*step", "step"), {"step": step})
            assert t1 == (step + 1) & M64
            assert _tuple(rr.advance_block(seed, t1, b)) == key + _source_counter(L, "advance", K, b=b, t1=t1)
            assert _tuple(rr.graph_block(seed, step, sweep, b, k, j)) == key + _source_counter(L, "graph", K, n=j, b=b, sweep=(sweep, 32),
                                                                                                 k=(k, 32), t=step)
            assert _tuple(rr.haar_block(seed, step)) == key + _source_counter(L, "haar", K, ctr=step)
            env = _env(K, t=step, b=b, j=j, M=M, N=N, n=j, k=(k, 32), sweep=(sweep, 32))
            env["gridDim.y"] = (B, 32)
            assert int(rr.tracker_fresh_offset(step, B, b, M, j)) == rr.c_eval(L["tracker_fresh"]["offset"], env)
            assert int(rr.graph_fresh_offset(step, sweep, b, k, N, j)) == rr.c_eval(L["graph_fresh"]["offset"], env)
            n += 1
    print("source expressions against the mirror: %d argument tuples x 8 layouts" % n)
    assert n >= 500


def test_c_eval_follows_c():
    ev = rr.c_eval
    assert ev("(unsigned)(t >> 32) << 16", {"t": 0x0001_8003_0000_0000}) == 0x80030000          # a 32-bit shift drops the top
    assert ev("(unsigned)b | ((unsigned)sweep << 16)", {"b": 5, "sweep": 255}) == 0x00FF0005
    assert ev("t * 256ull + 3ull", {"t": 2 ** 60}) == 3                                          # 64-bit wrap
    assert ev("a + b * c", {"a": 1, "b": 2, "c": 3}) == 7 and ev("(a + b) * c", {"a": 1, "b": 2, "c": 3}) == 9
    assert ev("a | b << 4", {"a": 1, "b": 1}) == 17 and ev("0x10u >> 4", {}) == 1
    assert ev("kTag | ((unsigned)k << 24)", {"kTag": (0x504752, 32), "k": (15, 32)}) == 0x0F504752


# ---- 3. the partition -----------------------------------------------------------------------------------------------------------
STREAM_TAGS = {"haar": rr.HAAR_TAG, "diffuse": rr.DIFFUSE_TAG, "velocity": rr.VELOCITY_TAG, "advance": rr.ADVANCE_TAG,
               "graph": rr.GRAPH_TAG}


def test_streams_differ_in_the_low_24_bits_of_word_2():
    pairs = 0
    for (a, ta), (b, tb) in itertools.combinations(STREAM_TAGS.items(), 2):
        assert (ta & 0xFFFFFF) != (tb & 0xFFFFFF), (a, b)
        pairs += 1
    assert pairs == 10 and all(0 < t < 1 << 24 for t in STREAM_TAGS.values())
    # whatever the arguments, word 2 keeps its tag there: the graph's node index sits above bit 24, the others have no field in it
    for k in range(16):
        assert _tuple(rr.graph_block(0, 0, 0, 0, k, 0))[4] & 0xFFFFFF == rr.GRAPH_TAG
        assert _tuple(rr.graph_block(0, 0, 0, 0, k, 0))[4] >> 24 == k


# left inverses: (key, counter) -> the arguments, modulo what the header says is dropped
def _seed_of(t):
    return t[0] | t[1] << 32


INVERSES = {
    "haar": (lambda seed, ctr: rr.haar_block(seed, ctr), lambda t: (_seed_of(t), t[2] | t[3] << 32), (64, 64), (64, 64)),
    "diffuse": (rr.diffuse_block, lambda t: (_seed_of(t), t[5] | (t[3] >> 16) << 32, t[3] & 0xFFFF, t[2]), (64, 64, 16, 31), (64, 48, 16, 31)),
    "velocity": (rr.velocity_block, lambda t: (_seed_of(t), t[5] | (t[3] >> 16) << 32, t[3] & 0xFFFF, t[2]), (64, 64, 16, 31), (64, 48, 16, 31)),
    "advance": (rr.advance_block, lambda t: (_seed_of(t), t[5] | t[3] << 32, t[2]), (64, 64, 16), (64, 64, 16)),
    "graph": (rr.graph_block, lambda t: (_seed_of(t), t[5] | (t[3] >> 24) << 32, (t[3] >> 16) & 0xFF, t[3] & 0xFFFF, t[4] >> 24, t[2]),
              (64, 64, 8, 16, 4, 31), (64, 40, 8, 16, 4, 31)),
}


@pytest.mark.parametrize("stream", sorted(INVERSES))
def test_stream_is_injective_over_its_ranges_and_wraps_where_stated(stream):
    """INVERSES[stream]: the layout, its left inverse, the width of every argument as passed and the width that enters the tuple.
    decode(encode(args)) == args modulo the kept widths proves injectivity there; flipping any kept bit changes the tuple, any
    dropped bit does not."""
    encode, decode, passed, kept = INVERSES[stream]
    rs = np.random.RandomState(sum(map(ord, stream)))
    values = [_probe_values(bits, rs, 3 if len(passed) >= 4 else 30) for bits in passed]
    probes = list(itertools.islice(itertools.product(*values), 0, None, max(1, int(np.prod([len(v) for v in values])) // 2400)))
    for args in probes:
        t = _tuple(encode(*args))
        assert t[4] & 0xFFFFFF == STREAM_TAGS[stream]
        assert decode(t) == tuple(a & ((1 << w) - 1) for a, w in zip(args, kept)), (stream, args)
    flipped = dropped = 0
    base = tuple(int(rs.randint(0, 2 ** 31)) % (1 << w) for w in passed)
    for i, (w, keep) in enumerate(zip(passed, kept)):
        for bit in range(w):
            other = tuple(a ^ (1 << bit) if m == i else a for m, a in enumerate(base))
            same = _tuple(encode(*other)) == _tuple(encode(*base))
            assert same == (bit >= keep), (stream, i, bit)
            flipped += not same
            dropped += same
    print("%-8s %d argument tuples through the left inverse; %d bits change the tuple, %d (dropped by the header) do not"
          % (stream, len(probes), flipped, dropped))
    assert dropped == sum(passed) - sum(kept) and len(probes) >= 1000


def test_noise_wraps_at_2p48_and_2p40_only():
    for step in (0, 1, 2 ** 32 + 1, 2 ** 47 + 3):
        for block in (rr.diffuse_block, rr.velocity_block):
            assert _tuple(block(9, step, 2, 100)) == _tuple(block(9, step + 2 ** 48, 2, 100))
            assert _tuple(block(9, step, 2, 100)) != _tuple(block(9, step + 2 ** 47, 2, 100))
        assert _tuple(rr.advance_block(9, step, 2)) != _tuple(rr.advance_block(9, step + 2 ** 48, 2))     # the counter whole
    for t in (0, 5, 2 ** 32 + 5, 2 ** 39 + 1):
        assert _tuple(rr.graph_block(9, t, 3, 2, 1, 100)) == _tuple(rr.graph_block(9, t + 2 ** 40, 3, 2, 1, 100))
        assert _tuple(rr.graph_block(9, t, 3, 2, 1, 100)) != _tuple(rr.graph_block(9, t + 2 ** 39, 3, 2, 1, 100))


def test_fresh_offsets_are_injective_within_their_family():
    """Both formulas are mixed-radix numbers -- digits j < M, b < B under `step`; n < N, k < 16, b < 65536, sweep < 256 under t --
    so divmod recovers the arguments from the exact value, and the value is exact (no wrap) while it stays below 2^64."""
    rs = np.random.RandomState(3)
    n = 0
    for B, M in ((1, 1), (1, 512), (3, 257), (65535, 2 ** 31 - 1), (7, 4099)):
        last = 2 ** 64 // (B * M) - 1                      # the largest step with (step + 1) B M <= 2^64
        for step in sorted({0, 1, min(2 ** 32 + 1, last), last // 2, last}):
            for b, j in ((0, 0), (B - 1, M - 1), (int(rs.randint(B)), int(rs.randint(M)))):
                off = int(rr.tracker_fresh_offset(step, B, b, M, j))
                rest, jj = divmod(off, M)
                assert (divmod(rest, B), jj) == ((step, b), j), (B, M, step, b, j)
                n += 1
        assert int(rr.tracker_fresh_offset(last + 1, B, B - 1, M, M - 1)) < (last + 2) * B * M - 1        # the next step has wrapped
    for N in (10, 257, 512, 2 ** 31 - 1):
        last = 2 ** 64 // (2 ** 28 * N) - 1
        for t in (0, 5, last // 2, last):
            for sweep, b, k, nn in ((0, 0, 0, 0), (255, 65535, 15, N - 1), (3, 2, 1, int(rs.randint(N)))):
                off = int(rr.graph_fresh_offset(t, sweep, b, k, N, nn))
                rest, n_ = divmod(off, N)
                rest, k_ = divmod(rest, 16)
                rest, b_ = divmod(rest, 65536)
                assert (divmod(rest, 256), b_, k_, n_) == ((t, sweep), b, k, nn), (N, t, sweep, b, k, nn)
                n += 1
    # the wrap the header states: modulo 2^64, so at N = 257 the graph's offsets repeat after 2^36 values of t
    assert int(rr.graph_fresh_offset(5, 3, 2, 1, 257, 200)) == int(rr.graph_fresh_offset(5 + 2 ** 36, 3, 2, 1, 257, 200))
    print("fresh offsets: %d argument tuples recovered by divmod" % n)


def test_the_recorded_overlap_of_tracker_and_graph_fresh_slots():
    """Same key (seed ^ 0x9E3779B97F4A7C15), same Haar tag, intersecting offsets: recorded, not changed -- the bytes of both
    families are pinned.  include/ahv.h tells the caller to give the two different seeds."""
    K = rr.source_constants()
    assert K["kFreshSeed"] == K["kGraphFreshSeed"] == rr.FRESH_XOR
    tracker = {int(rr.tracker_fresh_offset(1, 1, 0, 512, j)) for j in range(512)}
    graph = {int(rr.graph_fresh_offset(0, 0, 0, 1, 512, n)) for n in range(512)}
    assert tracker == graph == set(range(512, 1024))
    assert _tuple(rr.haar_block(77 ^ rr.FRESH_XOR, 600)) == _tuple(rr.haar_block(77 ^ rr.FRESH_XOR, 600))
    # a different seed separates them: the keys differ
    assert _tuple(rr.haar_block(77 ^ rr.FRESH_XOR, 600))[:2] != _tuple(rr.haar_block(78 ^ rr.FRESH_XOR, 600))[:2]


# ---- 4. the conditions of the GPU cases --------------------------------------------------------------------------------------------
def test_haar_cases_stay_away_from_a_vanishing_quaternion():
    for name in rc.HAAR_CASES:
        c = rc.haar_case(name)
        print("haar %-12s seed 0x%X (+%d) offset %d N %d: min |q| %.3f, e_ref %.2e" % (name, c.seed, c.seed_steps, c.offset, c.N, c.q_min, c.e_ref))
        assert c.q_min >= rc.HAAR_MIN_Q and c.e_ref > 0 and c.r32.dtype == np.float32 and c.r64.dtype == np.float64
    c = rc.haar_case("high_word")
    assert c.offset < 2 ** 32 <= c.offset + c.N - 1                         # the second counter word changes inside the call
    assert rc.haar_case("seed_high").seed >> 32 != 0
    name, lo, n = rc.SHARD
    assert lo + n == rc.haar_case(name).N


def test_noise_cases_meet_their_conditions():
    R, idx, V = rc.track_set()
    assert set(rr.shepperd_branch(R).tolist()) == {0, 1, 2, 3} and idx.shape == (rc.TRACK_B, rc.TRACK_M) and V.dtype == np.float32
    assert rc.TRACK_M > 256 and rc.diffuse_case("step_1").noise == slice(0, rc.TRACK_M)      # a noise slot in the second workgroup
    steps = set()
    for name in rc.DIFFUSE_CASES:
        c = rc.diffuse_case(name)
        steps.add(c.step)
        frac = float(c.clipped[:, c.noise].mean())
        print("diffuse %-10s seed 0x%X (+%d): branches %s, clipped %.2f, fresh min |q| %.3f" % (name, c.seed, c.seed_steps, sorted(c.branches), frac, c.fresh_q_min))
        assert c.branches == {0, 1, 2, 3} and c.fresh_q_min >= rc.HAAR_MIN_Q
        if c.max_angle_deg:
            assert 0.3 <= frac <= 0.7 and not c.near_band and c.same_decisions
        else:
            assert frac == 0
    assert steps == {1, 2 ** 32 + 1, 2 ** 47 + 3}
    for name in rc.PREDICT_CASES:
        c = rc.predict_case(name)
        fv, fp = float(c.clip_v[:, c.noise].mean()), float(c.clip_p[:, c.noise].mean())
        print("predict %-22s seed 0x%X (+%d): branches %s, |v'| clipped %.2f, |p| clipped %.2f" % (name, c.seed, c.seed_steps, sorted(c.branches), fv, fp))
        assert c.branches == {0, 1, 2, 3} and c.fresh_q_min >= rc.HAAR_MIN_Q
        if c.limits:
            assert 0 < fv < 1 and 0 < fp < 1 and not c.near_band and c.same_decisions
        else:
            assert fv == fp == 0
    assert {(c[2], c[3]) for c in rc.PREDICT_CASES.values()} >= {(True, True), (False, True), (True, False)}
    union = set()
    for name in rc.GRAPHS:
        for sweep in rc.GRAPH_SWEEPS:
            for t in rc.GRAPH_TS + (rc.GRAPH_WRAP + 5,):
                c = rc.graph_case(name, sweep, t)
                assert len(c.branches) == 3 and c.fresh_q_min >= rc.HAAR_MIN_Q      # three samples: three branches per graph
                assert c.noise.stop - c.noise.start > 150 and c.noise.start == 1 + c.D
        union |= c.branches
    assert union == {0, 1, 2, 3}
    assert {rc.GRAPHS[g][2] for g in rc.GRAPHS} >= {0, 15} and {rc.GRAPHS[g][3] for g in rc.GRAPHS} == {2, 8}


# ---- 5. the edge blocks, recomputed from their stored offsets ------------------------------------------------------------------------
def test_edge_blocks_hold_their_property():
    z, m, a = (rc.edge_case(k) for k in ("radius_zero", "radius_max", "angle_zero"))
    for k, c in (("radius_zero", z), ("radius_max", m), ("angle_zero", a)):
        print("edge %-11s offset %d: words %s, q %s, e_ref %.2e" % (k, c.offset, " ".join("%08x" % w for w in c.words), c.q64, c.e_ref))
        assert np.isfinite(c.r64).all() and np.isfinite(c.r32).all()
        assert np.abs(c.r64 @ c.r64.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    assert z.words[0] >> 8 == 0xFFFFFF
    for q in (z.q64, z.q32):
        assert q[0] == 0 and q[1] == 0 and np.hypot(q[2], q[3]) > 0.1          # radius exactly 0: a rotation about z
    assert m.words[0] >> 8 == 0
    assert np.isclose(np.hypot(m.q64[0], m.q64[1]), np.sqrt(48 * np.log(2)), rtol=1e-15)      # sqrt(-2 ln 2^-24) = 5.768
    assert a.words[1] >> 8 == 0
    for q in (a.q64, a.q32):
        assert q[1] == 0 and q[0] > 0                                           # angle exactly 0: sin = 0, cos = 1
