"""The device's random streams against the host mirror (tests/rng_reference.py): ``track_advance`` bit for bit, and
``random_rotations``, ``diffuse_rotations``, ``predict_rotations`` and ``pose_graph_propose`` against the mirror's fp64 values at
the (key, counter) tuples include/ahv.h states.  The cases and their conditions are tests/rng_cases.py's (tests/test_rng_cpu.py
asserts the conditions without a GPU).

The bar of every comparison that is not exact is tests/oplevel_cases.py's: over ALL slots of the case, the largest absolute entry
error against the fp64 mirror satisfies e_got <= 4 e_ref, e_ref being the fp32 mirror's own error on the same case.  A wrong
word, tag or bit field moves a value by O(1), a few ulp of logf / sincosf by a fraction of e_ref.  Every ratio is printed.

``track_advance`` is the one place the raw Philox output is visible: it pins rounds, multipliers, key schedule and which half
of the seed is which key word.  ``predict_rotations_controlled`` reading the same streams as the plain entry points, bit for bit
and in both kWalk forms, is asserted by tests/test_gpu_track_adapt.py::test_predict_follows_the_record_bit_for_bit and not
repeated here.

Edge blocks (tests/rng_cases.py EDGE_OFFSETS, found by tools/find_rng_edges.py): radius exactly 0, the largest radius, angle
exactly 0.  Both radii of a block being zero at once has probability 2^-48 per block and is not searched for: it is the one
input for which the sampler's quaternion vanishes (the matrix formula's clamp then gives the identity).

Figures measured on the MI355X, e_got / e_ref (this file prints them; DESIGN 4.2 quotes them):
  random_rotations      n4099 0.98, high_word 0.99, offset_2p40 0.98, seed_high 0.98, shard 1.04
  edge blocks           radius_zero 1.00, radius_max 1.00, angle_zero 1.56
  diffuse_rotations     omega 1.00 - 1.08, out 0.91 - 1.15, fresh slots 1.00 - 1.04 (2^48 + 1: 1.00)
  predict_rotations     vel_out 1.00 - 1.13, omega 1.00 - 1.02, out 0.81 - 0.96, fresh slots 0.99 - 1.01, p with v' = 0 1.02 - 1.03
  pose_graph_propose    30 launches: noise slots 0.68 - 1.05, fresh slots 0.92 - 1.14
  track_advance         45 launches, every word equal
No class needed an allowance beside the factor 4.  The file takes under 3 s.

That the tests bite: three throw-away builds with arithmetic-only changes, each run once over this file, tests/test_gpu_track.py,
tests/test_gpu_pose_graph.py and test_gpu_parity.py::test_device_haar_sampler (62 tests):
  philox4x32_10 with nine rounds      27 fail: all 26 of this file and test_gpu_track.py::test_random_rotations_bytes_are_unchanged
  the two key words swapped           27 fail: the same 27
  velocity block with the diffusion   3 fail: test_predict_velocity_and_noise_blocks_match_the_mirror, its three cases
  tag                                 (vel_out, omega and out all move by O(sigma_vel))
Every statistical, self-consistency and composition test of the older files passes on all three builds (the one older failure is
a byte pin): moments, bands and shard-equals-slice do not see a sampler that is wrong but still random.
"""
import numpy as np
import pytest
import torch

from . import rng_cases as rc
from . import rng_reference as rr

pytestmark = pytest.mark.gpu
MARGIN = 4.0            # tests/oplevel_cases.py
F64 = np.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


def _t(a):
    return torch.from_numpy(np.array(a))           # a copy: the cases' arrays are read-only


def _np(x):
    return x.detach().cpu().numpy()


def _counter(dev, value):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def accept(what, got, r32, r64):
    """The rule, over every element: e_got <= MARGIN e_ref.  Prints the figures first and returns e_got / e_ref."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and r32.dtype == np.float32 and r64.dtype == np.float64 and got.shape == r32.shape == r64.shape
    assert np.isfinite(got).all(), what + ": not finite"
    e_ref = float(np.abs(r32.astype(F64) - r64).max())
    e_got = float(np.abs(got.astype(F64) - r64).max())
    assert e_ref > 0.0, what + ": the fp32 mirror equals the fp64 one, no yardstick"
    print("%-64s e_got %.3e  e_ref %.3e  e_got/e_ref %.2f" % (what, e_got, e_ref, e_got / e_ref))
    assert e_got <= MARGIN * e_ref, "%s: e_got %.3e above %g x e_ref %.3e (ratio %.2f)" % (what, e_got, MARGIN, e_ref, e_got / e_ref)
    return e_got / e_ref


# ---- 1. track_advance: the raw Philox word ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", rc.ADVANCE_BATCHES)
def test_track_advance_is_the_first_philox_word(ops, dev, B):
    b = np.arange(B)
    for seed in rc.ADVANCE_SEEDS:
        for t in rc.ADVANCE_STEPS:
            step = _counter(dev, t)
            u = _np(ops.track_advance(step, seed, B))
            assert int(step.item()) == t + 1, (seed, t)
            want = rr.advance_u(seed, t + 1, b)
            assert u.dtype == np.float32 and np.array_equal(_bits(u), _bits(want)), (B, hex(seed), t, int((_bits(u) != _bits(want)).sum()))
            assert (u >= 0).all() and (u < 1).all()


# ---- 2. random_rotations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.HAAR_CASES))
def test_random_rotations_match_the_mirror(ops, dev, name):
    c = rc.haar_case(name)
    got = _np(ops.random_rotations(c.N, seed=c.seed, offset=c.offset, device=dev))
    accept("random_rotations %s (N %d, offset %d)" % (name, c.N, c.offset), got, c.r32, c.r64)


def test_a_shard_is_the_mirror_at_offset_plus_n(ops, dev):
    name, lo, n = rc.SHARD
    c = rc.haar_case(name)
    whole = ops.random_rotations(c.N, seed=c.seed, offset=c.offset, device=dev)
    shard = ops.random_rotations(n, seed=c.seed, offset=c.offset + lo, device=dev)
    assert torch.equal(shard, whole[lo:lo + n])
    accept("random_rotations shard [%d, %d) of %s" % (lo, lo + n, name), _np(shard), c.r32[lo:lo + n], c.r64[lo:lo + n])


@pytest.mark.parametrize("kind", sorted(rc.EDGE_OFFSETS))
def test_edge_blocks_of_box_muller(ops, dev, kind):
    c = rc.edge_case(kind)
    got = _np(ops.random_rotations(1, seed=rc.EDGE_SEED, offset=c.offset, device=dev))
    assert np.isfinite(got).all()
    G = got.astype(F64)[0]
    defect = float(np.abs(G @ G.T - np.eye(3)).max())
    print("edge %-11s offset %d: orthonormality defect %.2e, det - 1 %.2e" % (kind, c.offset, defect, np.linalg.det(G) - 1))
    assert defect < 5e-6 and abs(np.linalg.det(G) - 1) < 5e-6          # the bounds of test_device_haar_sampler
    accept("random_rotations edge block %s" % kind, got, c.r32, c.r64)


# ---- 3. diffuse_rotations ----------------------------------------------------------------------------------------------------------
def _track_inputs(dev):
    R, idx, V = rc.track_set()
    return _t(R).to(dev), _t(idx).to(dev), _t(V).to(dev)


def _diffuse(ops, dev, c, n_fresh, step=None, idx=None, R=None, seed=None):
    Rd, idxd, _ = _track_inputs(dev)
    return ops.diffuse_rotations(Rd if R is None else R, idx=idxd if idx is None else idx, sigma_deg=rc.TRACK_SIGMA_DEG,
                                 step=_counter(dev, c.step if step is None else step), seed=c.seed if seed is None else seed,
                                 n_fresh=n_fresh, max_angle_deg=c.max_angle_deg, want_omega=True)


@pytest.mark.parametrize("name", sorted(rc.DIFFUSE_CASES))
def test_diffuse_noise_and_fresh_slots_match_the_mirror(ops, dev, name):
    c = rc.diffuse_case(name)
    out, om = _diffuse(ops, dev, c, 0)                     # every slot a noise slot, the second workgroup's included
    accept("diffuse %s: omega against sigma z (step %d)" % (name, c.step), _np(om), c.omega32, c.omega64)
    accept("diffuse %s: out against R exp([omega]x)" % name, _np(out), c.out32, c.out64)
    if c.max_angle_deg:
        a = np.linalg.norm(_np(om).astype(F64), axis=-1)
        assert (a <= rc.rad32(c.max_angle_deg)).all() and rc._two_sided(c.clipped)
    outf, omf = _diffuse(ops, dev, c, rc.TRACK_FRESH)
    accept("diffuse %s: fresh slots against Haar at (step B + b) M + j" % name, _np(outf[:, c.fresh]), c.fresh32, c.fresh64)
    lo = rc.TRACK_M - rc.TRACK_FRESH
    assert not omf[:, c.fresh].any() and torch.equal(omf[:, :lo], om[:, :lo]) and torch.equal(outf[:, :lo], out[:, :lo])


def test_diffuse_noise_wraps_at_2p48_and_the_fresh_offset_does_not(ops, dev):
    """The header: the noise counter holds step[47:32] and step[31:0], so step + 2^48 repeats it bit for bit; the fresh offset
    takes step whole, so the fresh slots of step + 2^48 are other rotations -- the mirror's at ((step + 2^48) B + b) M + j."""
    c = rc.diffuse_case("step_1")
    wrapped = c.step + rc.TRACK_WRAP
    out, om = _diffuse(ops, dev, c, rc.TRACK_FRESH)
    outw, omw = _diffuse(ops, dev, c, rc.TRACK_FRESH, step=wrapped)
    lo = rc.TRACK_M - rc.TRACK_FRESH
    assert torch.equal(omw, om) and torch.equal(outw[:, :lo], out[:, :lo])
    assert not torch.equal(outw[:, lo:], out[:, lo:])
    f64 = rc._fresh(c.seed, wrapped, rc.TRACK_B, rc.TRACK_M, rc.TRACK_FRESH, np.float64)
    f32 = rc._fresh(c.seed, wrapped, rc.TRACK_B, rc.TRACK_M, rc.TRACK_FRESH, np.float32)
    accept("diffuse step 2^48 + 1: fresh slots against Haar at the whole step's offset", _np(outw[:, lo:]), f32, f64)
    # half the period is another block
    assert not torch.equal(_diffuse(ops, dev, c, 0, step=c.step + rc.TRACK_WRAP // 2)[1], _diffuse(ops, dev, c, 0)[1])


def test_diffuse_noise_of_a_slot_ignores_B_and_M(ops, dev):
    c = rc.diffuse_case("step_2p32")
    _, idx, _ = _track_inputs(dev)
    base = _diffuse(ops, dev, c, 0)[1]
    fewer_samples = _diffuse(ops, dev, c, 0, idx=idx[:2].contiguous())[1]                # B = 2, the same b
    assert torch.equal(fewer_samples, base[:2])
    more = torch.cat([idx, idx[-1:], idx[:1]]).contiguous()                               # B = 5
    assert torch.equal(_diffuse(ops, dev, c, 0, idx=more)[1][:3], base)
    fewer_slots = _diffuse(ops, dev, c, 0, idx=idx[:, :100].contiguous())[1]              # M = 100, the same j
    assert torch.equal(fewer_slots, base[:, :100])
    wider = torch.cat([idx, idx], dim=1).contiguous()                                     # M = 514
    assert torch.equal(_diffuse(ops, dev, c, 0, idx=wider)[1][:, :rc.TRACK_M], base)
    accept("diffuse B = 2: omega against the mirror's rows 0..1", _np(fewer_samples), c.omega32[:2], c.omega64[:2])
    accept("diffuse M = 100: omega against the mirror's slots 0..99", _np(fewer_slots), c.omega32[:, :100], c.omega64[:, :100])


# ---- 4. predict_rotations ----------------------------------------------------------------------------------------------------------
def _predict(ops, dev, c, n_fresh, **kw):
    Rd, idxd, Vd = _track_inputs(dev)
    args = dict(idx=idxd, sigma_deg=rc.TRACK_SIGMA_DEG, sigma_vel_deg=rc.TRACK_SIGMA_VEL_DEG, damping=rc.TRACK_DAMPING,
                step=_counter(dev, c.step), seed=c.seed, coast=False, n_fresh=n_fresh,
                max_angle_deg=rc.TRACK_MAX_ANGLE_DEG if c.limits else None, max_speed_deg=rc.TRACK_MAX_SPEED_DEG if c.limits else None,
                want_omega=True)
    args.update(kw)
    return ops.predict_rotations(Rd, Vd if c.with_V else None, **args)


@pytest.mark.parametrize("name", sorted(rc.PREDICT_CASES))
def test_predict_velocity_and_noise_blocks_match_the_mirror(ops, dev, name):
    c = rc.predict_case(name)
    out, vel, om = _predict(ops, dev, c, 0)
    accept("predict %s: vel_out against damping v + sigma_vel y" % name, _np(vel), c.vel32, c.vel64)
    accept("predict %s: omega against v' + p" % name, _np(om), c.omega32, c.omega64)
    accept("predict %s: out against R exp([omega]x)" % name, _np(out), c.out32, c.out64)
    if c.limits:
        assert (np.linalg.norm(_np(vel).astype(F64), axis=-1) <= rc.rad32(rc.TRACK_MAX_SPEED_DEG)).all()
    outf, velf, omf = _predict(ops, dev, c, rc.TRACK_FRESH)
    accept("predict %s: fresh slots against Haar at (step B + b) M + j" % name, _np(outf[:, c.fresh]), c.fresh32, c.fresh64)
    assert not omf[:, c.fresh].any() and not velf[:, c.fresh].any()


def test_predict_noise_is_the_block_diffuse_draws(ops, dev):
    """V None and sigma_vel = 0: v' = 0, so omega is p -- bit for bit the omega diffuse_rotations reports for (seed, step, b, j)."""
    for name in ("no_velocities_limits", "velocities_free"):
        c = rc.predict_case(name)
        Rd, idxd, _ = _track_inputs(dev)
        limit = rc.TRACK_MAX_ANGLE_DEG if c.limits else None
        out, vel, om = ops.predict_rotations(Rd, None, idx=idxd, sigma_deg=rc.TRACK_SIGMA_DEG, sigma_vel_deg=0.0, damping=rc.TRACK_DAMPING,
                                             step=_counter(dev, c.step), seed=c.seed, coast=False, max_angle_deg=limit,
                                             max_speed_deg=rc.TRACK_MAX_SPEED_DEG if c.limits else None, want_omega=True)
        outd, omd = ops.diffuse_rotations(Rd, idx=idxd, sigma_deg=rc.TRACK_SIGMA_DEG, step=_counter(dev, c.step), seed=c.seed,
                                          max_angle_deg=limit, want_omega=True)
        assert torch.equal(om, omd) and torch.equal(out, outd) and not vel.any(), name
        accept("predict %s, v' = 0: omega against the mirror's p" % name, _np(om), c.p32, c.p64)


# ---- 5. pose_graph_propose ---------------------------------------------------------------------------------------------------------
def _propose(ops, dev, name, sweep, t):
    V, edges, k, D = rc.GRAPHS[name]
    top = ops.PoseGraphTopology(V, None if edges is None else [tuple(e) for e in edges], 0, device=dev)
    assert top.degree[k] == D
    E = top.n_edges
    P = rr.haar_rotation(0xE0, np.arange(rc.GRAPH_B * E), np.float32).reshape(rc.GRAPH_B, E, 3, 3)
    s = (np.arange(rc.GRAPH_B * E, dtype=np.float32).reshape(rc.GRAPH_B, E) * np.float32(1e-2))
    A = _t(rc.graph_rotations(name)).to(dev)
    Q, _ = ops.pose_graph_propose(A, _t(P).to(dev), _t(s).to(dev), top, k, rc.GRAPH_N, rc.GRAPH_SIGMA_DEG, sweep=sweep, seed=rc.GRAPH_SEED,
                                  counter=_counter(dev, t), n_fresh=rc.GRAPH_FRESH)
    return Q


@pytest.mark.parametrize("name", sorted(rc.GRAPHS))
def test_pose_graph_candidates_match_the_mirror(ops, dev, name):
    for sweep in rc.GRAPH_SWEEPS:
        Qs = {}
        for t in rc.GRAPH_TS + (rc.GRAPH_WRAP + rc.GRAPH_TS[0],):
            c = rc.graph_case(name, sweep, t)
            Q = Qs[t] = _propose(ops, dev, name, sweep, t)
            what = "propose %s sweep %d t %d" % (name, sweep, t)
            accept(what + ": noise slots against A exp([sigma z]x)", _np(Q[:, c.noise]), c.q32, c.q64)
            accept(what + ": fresh slots against Haar at the header's offset", _np(Q[:, c.fresh]), c.fresh32, c.fresh64)
        # t[39:32] enters the noise counter: t + 2^40 repeats the noise bit for bit, t + 2^32 does not
        t0 = rc.GRAPH_TS[0]
        assert torch.equal(Qs[t0 + rc.GRAPH_WRAP][:, c.noise], Qs[t0][:, c.noise])
        assert not torch.equal(Qs[rc.GRAPH_TS[1]][:, c.noise], Qs[t0][:, c.noise])
