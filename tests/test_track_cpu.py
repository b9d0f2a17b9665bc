"""Pose tracking, CPU tier: argument validation of ``ahv_diffuse_rotations_f32`` / ``ahv_track_advance`` through the ctypes table
(validation runs before any HIP call), the host-side checks of the ops, ``track.PoseTracker``'s control flow on an oracle-backed
backend (tests/track_reference.py), ``harness.track_sequence`` on synthetic sequences, and the planted moving optimum."""
import os
import re

import numpy as np
import pytest
import torch

from . import track_reference as tr
from .conftest import REPO


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def _head(g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    return T("W1"), T("W2"), T("b2")


# ---- 1. the entry points refuse bad arguments before any HIP call ---------------------------------------------------
def test_diffuse_argument_validation_needs_no_gpu(lib):
    f = lib.ahv_diffuse_rotations_f32
    # (idx, R, r_batch_stride, N, best_key, M, n_fresh, B, seed, step, sigma, max_angle, out, omega, stream)
    ok = [None, 1, 0, 10, None, 8, 0, 2, 0, 1, 0.05, 0.0, 1, None, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(b"diffuse_rotations") and word in msg, (kw, msg)

    refused(b"null", _1=None)                    # R
    refused(b"null", _12=None)                   # out
    refused(b"null", _9=None)                    # step
    refused(b"M =", _5=0)
    refused(b"M =", _5=-3)
    refused(b"M =", _5=1 << 31)
    refused(b"empty rotation set", _3=0)
    refused(b"empty rotation set", _3=-1)
    refused(b"n_fresh", _6=-1)
    refused(b"n_fresh", _6=9)
    refused(b"B =", _7=0)
    refused(b"B =", _7=65536)
    refused(b"r_batch_stride", _2=9)
    refused(b"r_batch_stride", _2=89)
    refused(b"sigma", _10=-0.1)
    refused(b"sigma", _10=float("inf"))
    refused(b"sigma", _10=float("nan"))
    refused(b"max_angle", _11=-1.0)
    refused(b"max_angle", _11=float("inf"))
    refused(b"max_angle", _11=float("nan"))


def test_track_advance_argument_validation_needs_no_gpu(lib):
    f = lib.ahv_track_advance
    for args, word in (((0, None, 1, 1, None), b"null"), ((0, 1, 1, None, None), b"null"), ((0, 1, 0, 1, None), b"B ="),
                       ((0, 1, 65536, 1, None), b"B ="), ((0, 1, -2, 1, None), b"B =")):
        assert f(*args) == -1
        msg = lib.ahv_last_error()
        assert msg.startswith(b"track_advance") and word in msg, (args, msg)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ahv_diffuse_rotations_f32", "ahv_track_advance"):
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(ahv._lib.SIGNATURES[name][1]), name


# ---- 2. the ops check on the host ---------------------------------------------------------------------------------------
def test_ops_check_arguments_before_any_launch(ahv):
    ops = ahv.ops
    R = torch.eye(3)[None].repeat(4, 1, 1)
    step = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.diffuse_rotations(R, step=step)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_advance(step, 0, 2)
    with pytest.raises(RuntimeError, match="ONE element"):
        ops.track_advance(torch.zeros(2, dtype=torch.int64), 0, 2)
    with pytest.raises(RuntimeError, match="ONE element"):
        ops.track_advance(torch.zeros(1, dtype=torch.int32), 0, 2)
    with pytest.raises(RuntimeError, match="ONE element"):
        ops.track_advance(3, 0, 2)
    with pytest.raises(RuntimeError, match="finite and >= 0"):
        ops._angle_rad(-1.0, "sigma_deg")
    with pytest.raises(RuntimeError, match="finite and >= 0"):
        ops._angle_rad(float("nan"), "max_angle_deg", allow_none=True)
    assert ops._angle_rad(None, "max_angle_deg", allow_none=True) == 0.0
    assert ops._angle_rad(180.0, "x") == float(np.float32(np.pi))


def test_tracker_constructor_checks(ahv, g128):
    W1, W2, b2 = _head(g128)
    T = ahv.track.PoseTracker
    for kw, word in ((dict(particles=0), "particles"), (dict(particles=8, n_fresh=9), "n_fresh"), (dict(particles=8, batch=0), "batch"),
                     (dict(particles=8, sigma_deg=-1), "sigma_deg"), (dict(particles=8, temperature=0), "temperature"),
                     (dict(particles=8, max_angle_deg=float("inf")), "max_angle_deg"),
                     (dict(particles=8, posterior=True, mode_angle_deg=0.0), None)):
        with pytest.raises(RuntimeError, match=word):
            T(W1, W2, b2, **kw)
    t = T(W1, W2, b2, particles=8)
    with pytest.raises(RuntimeError, match="init"):
        t.step(torch.zeros(1, 16, 8, 8, 8), torch.zeros(1, 16, 8, 8, 8))


def test_use_graph_needs_the_hip_backend(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    with pytest.raises(RuntimeError, match="use_graph"):
        ahv.track.PoseTracker(W1, W2, b2, particles=8, use_graph=True)                                   # weights on the CPU
    with pytest.raises(RuntimeError, match="use_graph"):
        ahv.track.PoseTracker(W1, W2, b2, particles=8, use_graph=True, backend=tr.make_backend(ahv, oracle))


def test_init_keeps_its_own_copy_of_the_hypotheses(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(ahv, 1)

    def run(spoil):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=tr.make_backend(ahv, oracle))
        R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(16, seed=5))
        t.init(vs, vt, R0)
        if spoil:
            R0.zero_()
        return t.step(vs, vt).particles.clone()

    assert torch.equal(run(False), run(True))


# ---- 3. PoseTracker's control flow on the oracle backend ---------------------------------------------------------------
def _pair(ahv, B=2):
    g = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    return torch.from_numpy(g["vol_src"][:B]), torch.from_numpy(g["vol_tgt"][:B])


def test_tracker_control_flow(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    B, M, N0, F = 2, 24, 40, 5
    vs, vt = _pair(ahv, B)
    be = tr.make_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=4.0, n_fresh=F, temperature=0.05, batch=B, seed=3, backend=be)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    first = t.init(vs, vt, R0)
    assert first.draws is None and tuple(first.particles.shape) == (N0, 3, 3) and tuple(first.scores.shape) == (B, N0)
    assert torch.equal(first.idx, first.scores.argmax(dim=1)) and not first.reacquired.any()
    assert int(t.step_counter[0]) == 0
    prev, ptrs = first, {}
    for n in range(1, 7):
        be.calls.clear()
        out = t.step(vs, vt)
        assert be.calls == ["track_advance", "resample", "diffuse_rotations", "verify_pair", "select_rotation"]
        assert int(t.step_counter[0]) == n
        assert tuple(out.particles.shape) == (B, M, 3, 3) and tuple(out.scores.shape) == (B, M) and tuple(out.draws.shape) == (B, M)
        # the step is the mirror's, given the same random numbers
        draws, want = tr.mirror_step(prev.particles.numpy(), prev.scores.numpy(), M, 0.05, be.last_u, be.last_omega, be.last_fresh)
        assert np.array_equal(out.draws.numpy(), draws)
        assert np.array_equal(out.particles.numpy(), want.astype(np.float32))
        # the elite slot carries the previous arg-max, bit for bit; the fresh slots what the backend drew
        assert torch.equal(out.particles[:, 0], prev.R_map)
        assert np.array_equal(out.particles[:, M - F:].numpy(), be.last_fresh)
        # scores are the scorer's on the new set, and the winner is their arg-max
        s, _, _ = oracle.score_hypotheses(vs.numpy(), vt.numpy(), out.particles.numpy(), W1.numpy(), W2.numpy(), b2.numpy())
        assert np.array_equal(out.scores.numpy(), s)
        assert torch.equal(out.idx, out.scores.argmax(dim=1))
        assert torch.equal(out.R_map, out.particles[torch.arange(B), out.idx])
        assert torch.equal(out.reacquired, out.idx >= M - F)
        assert (out.score >= prev.score).all()          # same frame, elite kept: the score never decreases
        assert out.R_mean is None and out.entropy is None
        # ping-pong: a step writes the half the previous one did not, and after the first step nothing new appears
        now = tuple(x.data_ptr() for x in (out.score, out.idx, out.R_map, out.particles, out.scores, out.draws, out.reacquired))
        assert out.particles.data_ptr() != prev.particles.data_ptr() and out.scores.data_ptr() != prev.scores.data_ptr()
        if n >= 3:
            assert now == ptrs[n - 2], "a step allocated an output"
        if n >= 2:
            assert now[3] != ptrs[n - 1][3] and now[4] != ptrs[n - 1][4] and now[5] == ptrs[n - 1][5]
        ptrs[n] = now
        prev = out


def test_tracker_is_a_function_of_its_seed(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(ahv, 1)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(16, seed=5))

    def run(seed):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=seed, backend=tr.make_backend(ahv, oracle))
        t.init(vs, vt, R0)
        return [t.step(vs, vt).particles.clone() for _ in range(3)]

    a, b, c = run(1), run(1), run(2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])


# ---- 4. track_sequence ------------------------------------------------------------------------------------------------------
def test_track_sequence_on_synthetic_sequences(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    seqs = list(ahv.harness.SyntheticSequences(n_seq=2, n_frames=5, seed=3))
    vols = {}

    class Model:
        """Stands in for the encoder: a fixed random volume per frame (what is under test is the plumbing)."""

        def forward_features(self, a, b):
            f = lambda x: vols.setdefault(float(x.flatten()[0]), torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(len(vols))))
            return f(a), f(b)

    props = torch.from_numpy(ahv.rotations.haar_rotations_np(32, seed=9))
    for ref, item in zip((0, 2), seqs):
        t = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=tr.make_backend(ahv, oracle))
        res = ahv.harness.track_sequence(Model(), item, t, ref=ref, proposals=props, device="cpu")
        order = [k for k in range(5) if k != ref]
        assert res["frames"] == order
        assert tuple(res["R_map"].shape) == (4, 3, 3) and tuple(res["score"].shape) == (4,) and tuple(res["err"].shape) == (4,)
        assert int(t.step_counter[0]) == 3                      # init on the first tracked frame, a step on each of the rest
        for k, f in enumerate(order):
            R_gt = item["R"][f] @ item["R"][ref].T
            assert abs(float(res["err"][k]) - float(ahv.rotations.geodesic_deg(res["R_map"][k][None], R_gt[None]))) < 1e-4
        assert torch.isfinite(res["score"]).all() and (res["err"] >= 0).all() and (res["err"] <= 180).all()
    # row_vector_R: the annotation acts on row vectors (Co3dSequences), and the ground truth is evaluate_category's R_src^T R_tgt
    item, ref = seqs[0], 1
    run = lambda **kw: ahv.harness.track_sequence(
        Model(), item, ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=tr.make_backend(ahv, oracle)),
        ref=ref, proposals=props, device="cpu", **kw)
    col, row = run(), run(row_vector_R=True)
    assert torch.equal(col["R_map"], row["R_map"]) and not torch.equal(col["err"], row["err"])
    for k, f in enumerate(row["frames"]):
        R_gt = item["R"][ref].T @ item["R"][f]
        assert abs(float(row["err"][k]) - float(ahv.rotations.geodesic_deg(row["R_map"][k][None], R_gt[None]))) < 1e-4
    with pytest.raises(RuntimeError, match="batch = 1"):
        ahv.harness.track_sequence(Model(), seqs[0], ahv.track.PoseTracker(W1, W2, b2, particles=4, batch=2), device="cpu")


# ---- 5. the planted moving optimum ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_planted_moving_optimum(ahv, oracle, g128, s):
    """Measured on the oracle backend with numpy noise (tracker max over frames 6-11 / blind median over the 12 frames, degrees):
    1.20 / 8.44, 1.10 / 8.00 and 1.11 / 7.01 for s = 0, 1, 2."""
    P = tr.PLANTED
    W1, W2, b2 = _head(g128)
    vs = torch.from_numpy(np.ascontiguousarray(g128["vol_src"]))
    R0 = torch.from_numpy(tr.planted_init(ahv.rotations, s))
    w = [x.numpy() for x in (W1, W2, b2)]

    class T:
        def __init__(self):
            self.t = ahv.track.PoseTracker(W1, W2, b2, particles=P["particles"], sigma_deg=P["sigma_deg"], n_fresh=P["n_fresh"],
                                           temperature=P["temperature"], batch=1, seed=s, backend=tr.make_backend(ahv, oracle))

        def init_frame(self, vt):
            return self.t.init(vs, vt, R0)

        def step_frame(self, vt):
            return self.t.step(vs, vt)

    rotate = lambda R: torch.from_numpy(oracle.rotate_volume(vs.numpy(), R[None].astype(np.float32)))
    blind = lambda vt: R0.numpy()[int(oracle.score_hypotheses(vs.numpy(), vt.numpy(), R0.numpy(), *w)[2][0])]
    track, blind_err = tr.planted_run(ahv.rotations, s, rotate, T, blind)
    worst, median = tr.planted_bar(track, blind_err)
    print("planted s=%d: tracker %s | late max %.3f | blind %s | blind median %.3f"
          % (s, " ".join("%.2f" % e for e in track), worst, " ".join("%.1f" % e for e in blind_err), median))
    assert worst < median
