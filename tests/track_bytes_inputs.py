"""Inputs, and the one call sequence, of the recorded bytes of the tracking kernels (tests/golden/track_kernels_recorded.npz):
tools/gen_golden_track.py records what ``recompute`` yields and tests/test_gpu_track_bytes.py compares against it, so the fixture
holds outputs only.  The inputs are seeded numpy (``RandomState``) and ``rotations.haar_rotations_np``.

Smoothing chains: B = 2 (the ring's sample stride), H = 3 over 5 frames from ``first_step = 1`` (the ring wraps), M in ``MS`` --
one row, a ragged and a full 16-row workgroup, a ragged and a full 256-row tile, three tiles of which the last holds one row.
  "vel"    velocities (``hist_P``, damping 0.9), jump = 8
  "plain"  no velocities, jump = +inf
both at every M.
Planted: -inf and NaN scores; frame 2 of sample 1 without a finite score (a break: the frame after restarts); rows M // 3 and
M - 1 identical with the largest score (a tie that the first arg-max decides); one NaN matrix on a live row; sigma = 20 degrees,
at which some pairs of Haar rotations sit above the jump floor and some on it.
Predict step: B = 2, ``idx`` with -1 and N in it, every combination of the grid at M = 2, 255 and 257.  At the two large M a
covering choice of cases records the whole output and every other case the slots of ``edge_slots``: the elite, the coast slot, an
ordinary one and the last two (fresh with n_fresh = 2; at M = 257 they straddle the block edge 255 | 256).
"""
import importlib
import math

import numpy as np

rot = importlib.import_module("3dahv_amd.rotations")
dist = importlib.import_module("3dahv_amd.dist")

MS = (1, 15, 16, 17, 255, 256, 257, 513)
B, H, FRAMES, FIRST_STEP = 2, 3, 5, 1
TEMPERATURE, SIGMA_DEG, DAMPING = 0.05, 20.0, 0.9
CHAINS = {"vel": {"velocities": True, "jump": 8.0}, "plain": {"velocities": False, "jump": math.inf}}
HIST_P_MAX_M = 257
BREAK_FRAME, BREAK_SAMPLE, NAN_MATRIX_FRAME = 2, 1, 1

PREDICT_SEED, PREDICT_STEP = 0x1234ABCD5678, 5
PREDICT_MS, PREDICT_NS = (2, 255, 257), (1, 5)
# (M, N, best_key, n_fresh, max_angle_deg) of the diffuse cases and + (V: 0 absent / 1 shared / 2 per sample, coast) of the predict
# cases that record the whole output at the two large M; the others record ``edge_slots`` there
DIFFUSE_LARGE = {(255, 5, True, 2, 1.0), (257, 1, False, 0, None)}
PREDICT_LARGE = {(255, 5, True, 2, None, 2, True), (257, 1, True, 0, 1.0, 1, False)}
ADVANCE_B, ADVANCE_SEED, ADVANCE_STEP = 3, 0xC0FFEE12345, 4


def edge_slots(M):
    return [0, 1, 2, M - 2, M - 1]


def frames(M):
    """The FRAMES frames of the chains at M: a list of (R (B,M,3,3), scores (B,M), V (B,M,3)), float32."""
    rs = np.random.RandomState(7000 + M)
    out = []
    for f in range(FRAMES):
        R = rot.haar_rotations_np(B * M, seed=100 * M + f).reshape(B, M, 3, 3).copy()
        s = rs.uniform(-1.0, 1.0, (B, M)).astype(np.float32)
        V = (0.1 * rs.standard_normal((B, M, 3))).astype(np.float32)
        if f % 2:
            s[0, 3::7] = -np.inf
        else:
            s[1, 2::5] = np.nan
        if M == 1:
            s[0, 0] = {1: -np.inf, 3: np.nan}.get(f, s[0, 0])
        if M >= 2:
            a, c = M // 3, M - 1
            R[:, c], V[:, c] = R[:, a], V[:, a]
            s[:, a] = s[:, c] = 1.0
        if f == NAN_MATRIX_FRAME and M >= 3:
            R[0, 1] = np.nan
        if f == BREAK_FRAME:
            s[BREAK_SAMPLE, 0::2] = -np.inf
            s[BREAK_SAMPLE, 1::2] = np.nan
        out.append((R, s, V))
    return out


def predict_cases():
    """(name, kind, arguments, whole) of every recorded predict-step call; kind is "diffuse" or "predict", whole says whether
    the whole output is recorded or its ``edge_slots``."""
    for M in PREDICT_MS:
        for N in PREDICT_NS:
            for key in (False, True):
                for nf in (0, 2):
                    for ma in (None, 1.0):
                        yield ("diffuse_M%d_N%d_k%d_f%d_a%d" % (M, N, key, nf, ma is not None), "diffuse", (M, N, key, nf, ma),
                               M == 2 or (M, N, key, nf, ma) in DIFFUSE_LARGE)
                        for vmode in (0, 1, 2):
                            for coast in (False, True):
                                yield ("predict_M%d_N%d_k%d_f%d_a%d_v%d_c%d" % (M, N, key, nf, ma is not None, vmode, coast),
                                       "predict", (M, N, key, nf, ma, vmode, coast),
                                       M == 2 or (M, N, key, nf, ma, vmode, coast) in PREDICT_LARGE)


def predict_inputs(M, N, key, vmode):
    """R (per sample with a key, else shared), V or None, idx (B,M) with -1 and N in it, best_key (B,) or None."""
    rs = np.random.RandomState(31 * M + N)
    R = rot.haar_rotations_np(B * N, seed=500 + M + N).reshape(B, N, 3, 3)
    R = R if key else R[0]
    V = (0.05 * rs.standard_normal((B, N, 3))).astype(np.float32)
    V = None if vmode == 0 else V[0] if vmode == 1 else V
    idx = rs.randint(0, N, (B, M)).astype(np.int64)
    idx[0, 0], idx[-1, -1] = -1, N
    keys = None
    if key:
        keys = dist.pack_keys_host(np.array([0.5, 0.0], np.float32), np.array([N - 1, 0], np.int64)).copy()
        keys[1] = dist.KEY_EMPTY
    return np.ascontiguousarray(R), V, idx, keys


def unpack(recorded):
    """The fixture as {name: flat int32 words}."""
    ends = np.cumsum(recorded["sizes"])
    words = recorded["words"]
    return {str(n): words[e - k:e] for n, k, e in zip(recorded["names"], recorded["sizes"], ends)}


def _words(t):
    """Any tensor as its raw 32-bit words on the host."""
    import torch
    return t.detach().contiguous().cpu().view(torch.int32)


def recompute(ops, dev, M):
    """(name, int32 words) of everything recorded for the smoothing chains at M, from the library ``ops`` drives."""
    import torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    data = frames(M)
    for chain in CHAINS:
        cfg = CHAINS[chain]
        jump = cfg["jump"]
        hist = ops.smooth_history(B, M, H, dev, velocities=cfg["velocities"])
        marg = ops.marginal_history(B, M, H, dev)
        step = torch.zeros((1,), dtype=torch.int64, device=dev)
        pre = "M%d_%s_" % (M, chain)
        for f, (R, s, V) in enumerate(data):
            step.fill_(FIRST_STEP + f)
            Rd, sd = T(R), T(s)
            Vd = T(V) if cfg["velocities"] else None
            ops.smooth_step(hist, Rd, sd, step, TEMPERATURE, SIGMA_DEG, jump=jump, V=Vd, damping=DAMPING, first_step=FIRST_STEP)
            ops.marginal_step(hist, marg, Rd, sd, step, TEMPERATURE, SIGMA_DEG, jump=jump, first_step=FIRST_STEP)
            slot = (FIRST_STEP + f) % H
            yield pre + "f%d_delta" % f, _words(hist.delta[slot])
            yield pre + "f%d_back" % f, _words(hist.back[slot])
            yield pre + "f%d_alpha" % f, _words(marg.alpha[slot])
            yield "M%d_f%d_emit" % (M, f), _words(marg.emit[slot])      # beta s: the same in both chains
        if cfg["velocities"] and M <= HIST_P_MAX_M:
            yield pre + "hist_P", _words(hist.P)
        for F in (1, H):
            path = ops.smooth_backtrace(hist, step, frames=F, first_step=FIRST_STEP)
            yield pre + "path%d_idx" % F, _words(path.idx)
            yield pre + "path%d_R" % F, _words(path.R)
        for F in (1, 2, H):
            sm = ops.marginal_smooth(hist, marg, step, SIGMA_DEG, jump=jump, frames=F, first_step=FIRST_STEP)
            yield pre + "marg%d_logw" % F, _words(sm.logw)
            yield pre + "marg%d_idx" % F, _words(sm.idx)
            yield pre + "marg%d_R" % F, _words(sm.R)


def recompute_predict(ops, dev):
    """(name, int32 words) of the recorded predict-step calls and of ``track_advance``."""
    import torch
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    step = torch.full((1,), PREDICT_STEP, dtype=torch.int64, device=dev)
    for name, kind, args, whole in predict_cases():
        M, N, key, nf, ma = args[:5]
        pick = (lambda t: t) if whole else (lambda t: t[:, edge_slots(M)])
        R, V, idx, keys = predict_inputs(M, N, key, args[5] if kind == "predict" else 0)
        common = dict(idx=T(idx), sigma_deg=3.0, step=step, seed=PREDICT_SEED, best_key=T(keys), n_fresh=nf, max_angle_deg=ma,
                      want_omega=True)
        if kind == "diffuse":
            out, omega = ops.diffuse_rotations(T(R), **common)
        else:
            out, vel, omega = ops.predict_rotations(T(R), T(V), sigma_vel_deg=1.0, damping=DAMPING, coast=args[6],
                                                    max_speed_deg=None if ma is None else 2.0, **common)
            yield name + "_vel", _words(pick(vel))
        yield name + "_out", _words(pick(out))
        yield name + "_omega", _words(pick(omega))
    step = torch.full((1,), ADVANCE_STEP, dtype=torch.int64, device=dev)
    for k in range(2):
        yield "advance%d_u" % k, _words(ops.track_advance(step, ADVANCE_SEED, ADVANCE_B))
    yield "advance_step", _words(step)
