"""Pose selection modulo a symmetry group, CPU tier: the reference's own maths (tests/sym_reference.py: the closed form against a
scan over the axis angle), ``rotations.Symmetry`` and ``geodesic_sym_deg``, argument validation of ``ahv_sym_fold_f32`` /
``ahv_topk_modes_sym_f32`` through the ctypes table (validation runs before any HIP call), the host-side checks of the ops,
``PoseTracker(symmetry=)``'s control flow on an oracle-backed backend, and ``harness.test_linemod_category(symmetry="config")``."""
import math
import os
import re

import numpy as np
import pytest
import torch

from . import sym_reference as sr
from . import track_reference as tr
from .conftest import REPO


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def _groups(ahv):
    Sy = ahv.rotations.Symmetry
    return {"trivial": Sy.trivial_group(), "c2": Sy.cyclic(2), "c5": Sy.cyclic(5, (1.0, -2.0, 0.5)), "d2": Sy.dihedral(2, "X"),
            "d3": Sy.dihedral(3, (1.0, 1.0, 0.0)), "tetra": Sy.tetrahedral(), "octa": Sy.octahedral(), "icosa": Sy.icosahedral(),
            "cinf": Sy.axial((2.0, -1.0, 2.0)), "dinf": Sy.axial("Y", flip=True)}


def _np(sym):
    return sym.S.numpy(), (None if sym.axis is None else sym.axis.numpy())


# ---- the reference's maths ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", [False, True])
def test_closed_form_against_a_scan_over_phi(ahv, flip):
    """max over phi of tr(M Rot(a, phi)) = p + sqrt(c^2 + s^2) at cos phi = c / h, sin phi = s / h -- value and the SIGN of phi --
    against a dense scan in fp64."""
    sym = ahv.rotations.Symmetry.axial((1.0, 2.0, 3.0), flip=flip)
    S, a = (x.astype(np.float64) for x in _np(sym))
    R = ahv.rotations.haar_rotations_np(64, 1).astype(np.float64)
    A = ahv.rotations.haar_rotations_np(1, 2)[0].astype(np.float64)
    t, g, cphi, sphi, _ = sr.sym_trace(R, A, S, a)
    phis = np.linspace(-math.pi, math.pi, 7201)
    rots = sr.rot(a, np.cos(phis), np.sin(phis))                                   # (P,3,3)
    vals = np.einsum("nij,gjk,pkl,il->ngp", R, S, rots, A)                          # <R S_g Rot(phi), A>
    assert np.abs(vals.reshape(64, -1).max(axis=1) - t).max() < 2e-7               # half a grid step is 4.4e-4 rad: h (1 - cos) <= 2 x 9.5e-8
    for n in range(64):
        gb, pb = np.unravel_index(np.argmax(vals[n]), vals[n].shape)
        assert gb == g[n]
        phi_star = math.atan2(sphi[n], cphi[n])
        d = (phis[pb] - phi_star + math.pi) % (2 * math.pi) - math.pi
        assert abs(d) <= 0.5 * (phis[1] - phis[0]) + 1e-9                          # the scan's best angle is the grid point nearest phi*
        # and the value AT phi* is the closed form to rounding
        Q = S[g[n]] @ sr.rot(a, np.array([cphi[n]]), np.array([sphi[n]]))[0]
        assert abs(np.sum((R[n] @ Q) * A) - t[n]) < 4e-15
    assert abs(cphi ** 2 + sphi ** 2 - 1).max() < 1e-15


def test_fold_moves_to_the_nearest_member_of_the_orbit(ahv):
    """The folded hypothesis has plain trace t_G against its anchor, and no other group element does better."""
    for name, sym in _groups(ahv).items():
        S, a = _np(sym)
        R = ahv.rotations.haar_rotations_np(50, 3)
        A = ahv.rotations.haar_rotations_np(2, 4)[None]
        V = np.random.default_rng(0).standard_normal((1, 50, 3)).astype(np.float32)
        f = sr.fold(R, S, a, A, None, 0, V)
        assert np.all(f["which"] == 0) and np.all(f["elem"] >= 0), name
        plain = np.einsum("nij,ij->n", f["R"][0], A[0, 0].astype(np.float64))
        assert np.abs(plain - f["trace"][0]).max() < 1e-6, name                    # (S is fp32-rounded: closure to ~1e-7)
        again = sr.fold(f["R"][0], S, a, A, None, 0)                                # folding twice moves nothing further
        assert np.abs(again["trace"] - f["trace"]).max() < 1e-6, name
        assert np.abs(np.linalg.norm(f["V"], axis=-1) - np.linalg.norm(V, axis=-1)).max() < 1e-6, name
        lim = sr.fold(R, S, a, A, 15.0, 3, V)                                        # with a limit: few fold, keep slots never
        assert np.all(lim["which"][:, :3] == -1) and np.array_equal(lim["R"][0, :3], R[:3].astype(np.float64))
        hit = lim["which"] >= 0
        assert np.all(lim["trace"][hit] >= sr.tau_of(15.0)) and np.all(np.isnan(lim["trace"][~hit]))


def test_mode_selection_of_the_trivial_group_is_the_plain_one(ahv):
    from . import modes_reference as mr
    rng = np.random.default_rng(5)
    s = rng.standard_normal((2, 300)).astype(np.float32)
    R = ahv.rotations.haar_rotations_np(300, 6)
    S, a = _np(ahv.rotations.Symmetry.trivial_group())
    k0, m0 = mr.select_modes(s, R, 16, 40.0, n_offset=5)
    k1, m1 = sr.select_modes(s, R, 16, 40.0, S, a, n_offset=5)
    assert np.array_equal(k0, k1) and m0 == m1
    # a group: a subsequence of the plain list's candidates, never longer
    k2, _ = sr.select_modes(s, R, 16, 40.0, *_np(ahv.rotations.Symmetry.octahedral()), n_offset=5)
    assert ((k2 != sr.EMPTY).sum(1) <= (k0 != sr.EMPTY).sum(1)).all() and np.array_equal(k2[:, 0], k0[:, 0])


# ---- rotations.Symmetry ------------------------------------------------------------------------------------------------

def test_group_constructors(ahv):
    g = _groups(ahv)
    orders = {"trivial": 1, "c2": 2, "c5": 5, "d2": 4, "d3": 6, "tetra": 12, "octa": 24, "icosa": 60, "cinf": 1, "dinf": 2}
    for name, sym in g.items():
        assert sym.order == orders[name] and sym.S.dtype == torch.float32, name
        assert torch.equal(sym.S[0], torch.eye(3)), name
        S = sym.S.double()
        # closure, again and independently of the constructor's own check (which every constructor has passed to get here)
        P = (S[:, None] @ S[None]).reshape(-1, 1, 3, 3)
        assert float((P - S[None]).flatten(-2).norm(dim=-1).min(dim=-1).values.max()) < 1e-6, name
        assert float((torch.linalg.det(S) - 1).abs().max()) < 1e-6, name
        type(sym)(sym.S, sym.axis)   # passes its own check
    assert (g["cinf"].axis is not None) and (g["dinf"].axis is not None) and g["octa"].axis is None
    assert set(np.unique(g["octa"].S.numpy()).tolist()) == {-1.0, 0.0, 1.0}        # exact cube rotations
    Sy = ahv.rotations.Symmetry
    assert torch.equal(Sy.from_config(["Z", 180]).S, Sy.cyclic(2, "Z").S) and Sy.from_config(["Z", 180]).order == 2
    assert Sy.from_config(["X", 90]).order == 4 and Sy.from_config(["y", 0]).axis is not None
    with pytest.raises(ValueError, match="divide"):
        Sy.from_config(["Z", 100])


def test_symmetry_refuses_what_is_no_group(ahv):
    Sy = ahv.rotations.Symmetry
    c4 = Sy.cyclic(4).S
    with pytest.raises(ValueError, match="closed"):
        Sy(c4[:3])                                                   # identity, 90, 180 degrees: 270 is missing
    with pytest.raises(ValueError, match="identity"):
        Sy(c4[[1, 0, 2, 3]])                                         # a group, but element 0 is not the identity
    nearly = c4.clone()
    nearly[0, 0, 0] = 1.0 + 2.0 ** -23
    with pytest.raises(ValueError, match="identity"):
        Sy(nearly)                                                   # the identity EXACTLY
    with pytest.raises(ValueError, match="rotation"):
        Sy(torch.stack([torch.eye(3), torch.diag(torch.tensor([1.0, 1.0, -1.0]))]))   # a reflection
    with pytest.raises(ValueError, match="G = 65"):
        Sy(torch.eye(3)[None].repeat(65, 1, 1))
    with pytest.raises(ValueError, match="G = 0"):
        Sy(torch.zeros(0, 3, 3))
    Sy.cyclic(64)                                                    # G = 64 is the largest
    with pytest.raises(ValueError, match="axis"):
        Sy(Sy.cyclic(2, "X").S, torch.tensor([0.6, 0.8, 0.0]))       # the half turn about X maps this axis elsewhere
    Sy(Sy.cyclic(2, "X").S, torch.tensor([0.0, 0.0, 1.0]))           # ... but Z to -Z: D_inf
    with pytest.raises(ValueError, match="unit"):
        Sy(torch.eye(3)[None], torch.tensor([0.0, 0.0, 2.0]))
    off = Sy.cyclic(3).S.clone()
    off[1] = off[1] @ ahv.rotations.axis_angle_to_matrix(torch.tensor([[2e-5, 0.0, 0.0]]))[0]
    with pytest.raises(ValueError, match="closed"):
        Sy(off)                                                      # 2e-5 rad off: outside the 1e-5 tolerance


def test_conjugate_and_to(ahv):
    Sy = ahv.rotations.Symmetry
    P = torch.from_numpy(ahv.rotations.haar_rotations_np(3, 9))
    for sym in (Sy.octahedral(), Sy.axial("Z", flip=True)):
        c = sym.conjugate(P)
        assert tuple(c.S.shape) == (3, sym.order, 3, 3) and torch.equal(c.S[:, 0], torch.eye(3).expand(3, 3, 3))
        want = P.double()[:, None] @ sym.S.double()[None] @ P.double().transpose(-1, -2)[:, None]
        assert float((c.S.double() - want).abs().max()) < 1e-7
        one = sym.conjugate(P[1])
        assert tuple(one.S.shape) == (sym.order, 3, 3) and torch.equal(one.S, c.S[1])
        if sym.axis is not None:
            assert tuple(c.axis.shape) == (3, 3) and float((c.axis.double() - (P.double() @ sym.axis.double())).abs().max()) < 1e-7
        assert c.to("cpu").S.data_ptr() == c.S.data_ptr()
    with pytest.raises(ValueError, match="disagree"):
        Sy.octahedral().conjugate(P).conjugate(P[:2])


def test_geodesic_sym_deg(ahv):
    geo, geo_sym = ahv.rotations.geodesic_deg, ahv.rotations.geodesic_sym_deg
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(40, 1)).double()
    Rg = torch.from_numpy(ahv.rotations.haar_rotations_np(40, 2)).double()
    assert torch.equal(geo_sym(R, Rg, None), geo(R, Rg))
    assert torch.equal(geo_sym(R, Rg, ahv.rotations.Symmetry.trivial_group()), geo(R, Rg))
    for name, sym in _groups(ahv).items():
        d = geo_sym(R, Rg, sym)
        assert bool((d <= geo(R, Rg) + 1e-9).all()), name
        for g in range(0, sym.order, 7):
            # arccos near 1: an error of 1e-7 in the trace (the fp32-rounded group) is 0.03 degrees
            assert float(geo_sym(R @ sym.S[g].double(), R, sym).max()) < 0.05, name
        S, a = _np(sym)
        t = np.stack([sr.sym_trace(R[i:i + 1].numpy(), Rg[i].numpy(), S, a)[0][0] for i in range(40)])
        want = np.degrees(np.arccos((np.clip(t, -1, 3) - 1) / 2))
        assert np.abs(d.numpy() - want).max() < 1e-6, name
    sym = ahv.rotations.Symmetry.axial("Z")
    turn = ahv.rotations.axis_angle_to_matrix(torch.tensor([[0.0, 0.0, 1.234]], dtype=torch.float64))[0]
    assert float(geo_sym(R @ turn, R, sym).max()) < 0.05 and float(geo(R @ turn, R).min()) > 70.0
    per = sym.conjugate(R[:40].float())    # per-sample groups
    assert tuple(geo_sym(R, Rg, per).shape) == (40,)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------

def _caller(lib, f, ok, prefix):
    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(prefix) and word in msg, (kw, msg)
    return call, refused


def test_sym_fold_argument_validation_needs_no_gpu(lib):
    # (R, r_batch_stride, B, N, S, s_batch_stride, G, axis, axis_batch_stride, anchors, K, min_trace, keep, V, R_out, V_out, which,
    #  elem, trace, stream)
    tau = sr.tau_of(15.0)
    ok = [1, 0, 2, 10, 1, 0, 4, None, 0, 1, 3, tau, 0, None, 1, None, None, None, None, None]
    call, refused = _caller(lib, lib.ahv_sym_fold_f32, ok, b"sym_fold")
    for bad in (0, 65, -1):
        refused(b"G =", _6=bad)
    for bad in (0, 17, -2):
        refused(b"K =", _10=bad)
    for bad in (5, 89, 91, -90):
        refused(b"r_batch_stride", _1=bad)
    for bad in (9, 35, 37, -36):
        refused(b"s_batch_stride", _5=bad)
    for bad in (1, 2, 4, -3):
        refused(b"axis_batch_stride", _8=bad)
    for bad in (-1.0, 3.0, float("nan"), float("inf"), 3.5, -1.5):
        refused(b"min_trace", _11=bad)
    for bad in (-1, 11):
        refused(b"keep", _12=bad)
    refused(b"null", _0=None)
    refused(b"null", _4=None)
    refused(b"null", _9=None)
    refused(b"null", _14=None)
    refused(b"go together", _13=1)
    refused(b"go together", _15=1)
    refused(b"negative", _2=-1)
    refused(b"negative", _3=-1)
    refused(b"65535", _2=65536)
    assert call(_2=0, _0=None, _14=None) == 0 and call(_3=0, _12=0, _0=None, _14=None) == 0   # B = 0 / N = 0: nothing to do
    refused(b"keep", _3=0, _12=1)


def test_topk_modes_sym_argument_validation_needs_no_gpu(lib):
    # (scores, R, r_batch_stride, B, N, n_offset, K, min_trace, S, s_batch_stride, G, axis, axis_batch_stride, keys, workspace,
    #  workspace_bytes, stream)
    tau = sr.tau_of(15.0)
    ok = [1, 1, 0, 1, 10, 0, 4, tau, 1, 0, 4, None, 0, 1, 16, 1 << 20, None]
    call, refused = _caller(lib, lib.ahv_topk_modes_sym_f32, ok, b"topk_modes_sym")
    for bad in (0, 65, -1):
        refused(b"K =", _6=bad)
        refused(b"G =", _10=bad)
    for bad in (-1.0, 3.0, float("nan"), float("inf"), -float("inf")):
        refused(b"min_trace", _7=bad)
    for bad in (5, 89, 91):
        refused(b"r_batch_stride", _2=bad)
    for bad in (9, 35, 37):
        refused(b"s_batch_stride", _9=bad)
    for bad in (1, 4):
        refused(b"axis_batch_stride", _12=bad)
    refused(b"null", _0=None)
    refused(b"null", _1=None)
    refused(b"null", _8=None)
    refused(b"null", _13=None)
    refused(b"negative", _4=-10)
    refused(b"65535", _3=65536)
    refused(b"32 bits", _5=1 << 32)
    refused(b"workspace", _14=None, _15=0)
    refused(b"workspace", _15=8 * 12 - 1)
    refused(b"aligned", _14=24)
    assert call(_3=0, _0=None, _1=None, _13=None, _14=None, _15=0) == 0   # B = 0: nothing to do


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3   # added under 2.3: callers probe for the symbol
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("ahv_sym_fold_f32", "ahv_topk_modes_sym_f32"):
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(ahv._lib.SIGNATURES[name][1]), name
    assert ahv._lib.AHV_SYM_MAX_ELEMENTS == 64 == ahv.rotations.SYM_MAX_ELEMENTS and ahv._lib.AHV_SYM_FOLD_MAX_ANCHORS == 16


def test_ops_refuse_cpu_tensors_and_bad_arguments(ahv):
    ops, Sy = ahv.ops, ahv.rotations.Symmetry
    R = torch.eye(3)[None].repeat(8, 1, 1)
    anchors = torch.eye(3)[None, None].repeat(2, 3, 1, 1)
    sym = Sy.cyclic(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sym_fold(R, sym, anchors)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_modes(torch.zeros(2, 8), R, 4, 15.0, symmetry=sym)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_posterior(torch.zeros(2, 8), R, anchors=anchors, min_angle_deg=15.0, symmetry=sym)
    with pytest.raises(RuntimeError, match="needs anchors"):
        ops.pose_posterior(torch.zeros(2, 8), R, symmetry=sym)
    with pytest.raises(RuntimeError, match="K = 17"):
        ops.sym_fold(R, sym, torch.eye(3)[None, None].repeat(2, 17, 1, 1))
    with pytest.raises(RuntimeError, match="keep"):
        ops.sym_fold(R, sym, anchors, keep=9)
    with pytest.raises(RuntimeError, match="min_angle_deg"):
        ops.sym_fold(R, sym, anchors, min_angle_deg=180.0)
    with pytest.raises(RuntimeError, match="anchors must be"):
        ops.sym_fold(R, sym, torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="rotations.Symmetry"):
        ops.topk_modes(torch.zeros(2, 8), R, 4, 15.0, symmetry="Z")


def test_coarse_to_fine_takes_symmetry_with_modes_only(ahv, g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(32, 1))
    sym = ahv.rotations.Symmetry.cyclic(2)
    for kw in (dict(), dict(seeds=4), dict(resample=True)):
        with pytest.raises(RuntimeError, match="symmetry"):
            ahv.refine.CoarseToFine(T("W1"), T("W2"), T("b2"), R, n_fine=8, symmetry=sym, backend=object(), **kw)


# ---- PoseTracker(symmetry=) on the oracle backend ---------------------------------------------------------------------------

def _sym_backend(ahv, oracle):
    """tests/track_reference.py's backend (imported, not edited) with ``sym_fold`` as the numpy reference."""
    base = tr.make_backend(ahv, oracle)

    class SymBackend(type(base)):
        def sym_fold(self, R, symmetry, anchors, min_angle_deg=None, keep=0, V=None, out=None, V_out=None, want_info=True):
            assert out is not None and out.data_ptr() == R.data_ptr() and not want_info       # in place, nothing allocated
            self.fold_args = (R.clone(), anchors.clone(), keep, None if V is None else V.clone())
            f = sr.fold(R.numpy(), symmetry.S.numpy(), None if symmetry.axis is None else symmetry.axis.numpy(), anchors.numpy(),
                        min_angle_deg, keep, None if V is None else V.numpy())
            new = np.where(f["moved"][..., None, None], f["R"].astype(np.float32), R.numpy())
            out.copy_(torch.from_numpy(new))
            if V is not None:
                assert V_out is not None and V_out.data_ptr() == V.data_ptr()
                V_out.copy_(torch.from_numpy(np.where(f["moved"][..., None], f["V"].astype(np.float32), V.numpy())))
            self.calls.append("sym_fold")
            return ahv.ops.SymFold(out, None, None, None, V_out)

    return SymBackend()


def _head(g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    return T("W1"), T("W2"), T("b2")


def _pair(B=2):
    g = np.load(os.path.join(REPO, "tests", "golden", "batched.npz"))
    return torch.from_numpy(g["vol_src"][:B]), torch.from_numpy(g["vol_tgt"][:B])


def test_tracker_folds_between_predict_and_verify(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    B, M, N0, F = 2, 24, 40, 5
    vs, vt = _pair(B)
    sym = ahv.rotations.Symmetry.dihedral(2, "Z").conjugate(torch.from_numpy(ahv.rotations.haar_rotations_np(B, 2)))
    be = _sym_backend(ahv, oracle)
    t = ahv.track.PoseTracker(W1, W2, b2, particles=M, sigma_deg=4.0, n_fresh=F, temperature=0.05, batch=B, seed=3, backend=be,
                              symmetry=sym)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(N0, seed=5))
    prev = t.init(vs, vt, R0)
    S = sym.S.numpy().astype(np.float64)
    for n in range(1, 5):
        be.calls.clear()
        out = t.step(vs, vt)
        assert be.calls == ["track_advance", "resample", "diffuse_rotations", "sym_fold", "verify_pair", "select_rotation"]
        R_in, anchors, keep, V = be.fold_args
        assert keep == 1 and V is None and tuple(anchors.shape) == (B, 1, 3, 3)
        assert torch.equal(anchors[:, 0], prev.R_map)                              # the previous frame's MAP pose, no limit
        # the unfolded set is the mirror's; the step's particles are its fold: one fundamental domain around the anchor
        _, want = tr.mirror_step(prev.particles.numpy(), prev.scores.numpy(), M, 0.05, be.last_u, be.last_omega, be.last_fresh)
        assert np.array_equal(R_in.numpy(), want.astype(np.float32))
        assert torch.equal(out.particles[:, 0], prev.R_map)                        # the elite: bit for bit
        for b in range(B):
            tG = sr.sym_trace(out.particles[b, 1:].numpy(), prev.R_map[b].numpy(), S[b])[0]
            plain = np.einsum("nij,ij->n", out.particles[b, 1:].numpy().astype(np.float64), prev.R_map[b].numpy().astype(np.float64))
            assert np.abs(tG - plain).max() < 1e-5                                 # no equivalent pose is nearer the anchor
        s, _, _ = oracle.score_hypotheses(vs.numpy(), vt.numpy(), out.particles.numpy(), W1.numpy(), W2.numpy(), b2.numpy())
        assert np.array_equal(out.scores.numpy(), s)                               # the scorer saw the FOLDED set
        assert torch.equal(out.R_map, out.particles[torch.arange(B), out.idx])
        prev = out


def test_tracker_symmetry_needs_a_backend_with_sym_fold_and_none_is_the_old_tracker(ahv, oracle, g128):
    W1, W2, b2 = _head(g128)
    vs, vt = _pair(1)
    sym = ahv.rotations.Symmetry.cyclic(2)
    with pytest.raises(RuntimeError, match="sym_fold"):
        ahv.track.PoseTracker(W1, W2, b2, particles=8, backend=tr.make_backend(ahv, oracle), symmetry=sym)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(16, seed=5))

    def run(**kw):
        be = _sym_backend(ahv, oracle)
        t = ahv.track.PoseTracker(W1, W2, b2, particles=16, batch=1, seed=1, backend=be, **kw)
        t.init(vs, vt, R0)
        outs = [t.step(vs, vt) for _ in range(3)]
        return be.calls, torch.stack([o.particles.clone() for o in outs])

    calls0, p0 = run()
    calls1, p1 = run(symmetry=None)
    calls2, p2 = run(symmetry=ahv.rotations.Symmetry.trivial_group())
    assert "sym_fold" not in calls0 and calls0 == calls1 and torch.equal(p0, p1)
    assert calls2.count("sym_fold") == 3 and torch.equal(p0, p2)                   # the trivial group folds nothing


# ---- harness.test_linemod_category(symmetry="config") ----------------------------------------------------------------

class _FlippedModel:
    """Predicts the ground truth turned by exactly the object's 180 degree symmetry about Z (in the source view's frame)."""
    num_rota = 4

    def __call__(self, src_img, src_mask, ref_img, ref_mask):
        return src_img, ref_img            # (the "volumes" carry the poses: see the loader)

    def verify(self, vol_src, vol_tgt, codebook):
        P_src, P_ref = vol_src, vol_tgt
        flip = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=P_src.dtype))
        return None, None, None, P_ref @ flip @ P_src.transpose(-1, -2)


def _linemod_loader(ahv, batches=3, B=4):
    for k in range(batches):
        P = torch.from_numpy(ahv.rotations.haar_rotations_np(2 * B, 40 + k)).double()
        mask = torch.ones(B, 1, 8, 8)
        yield {"src_mask": mask, "ref_mask": mask, "src_img": P[:B], "ref_img": P[B:], "src_R": P[:B], "ref_R": P[B:]}


def test_linemod_category_scores_a_symmetric_answer_as_correct(ahv, tmp_path):
    cfg = {"DATA": {"SIZE_THR": 1}, "RUN_NAME": "x", "LINEMOD": {"SYMMETRIC_OBJ": {"000010": ["Z", 180], "000011": ["Z", 180]}}}
    run = lambda clsID, **kw: ahv.harness.test_linemod_category(cfg, _FlippedModel(), _linemod_loader(ahv), clsID,
                                                                 out_dir=str(tmp_path), **kw)
    err, acc30, acc15 = run(10)
    assert acc15 == 0.0 and acc30 == 0.0 and abs(err - 180.0) < 0.1                # the reference's metric: 180 degrees off
    err, acc30, acc15 = run(10, symmetry="config")
    assert acc15 == 100.0 and acc30 == 100.0 and err < 0.1       # (arccos near 1: the fp32-rounded group leaves ~0.02 degrees)
    err, acc30, acc15 = run(5, symmetry="config")                                   # no entry for this object: no symmetry
    assert acc15 == 0.0
    err, acc30, acc15 = run(5, symmetry=ahv.rotations.Symmetry.cyclic(2, "Z"))      # a Symmetry in the object's frame
    assert acc15 == 100.0
    with pytest.raises(ValueError, match="config"):
        run(10, symmetry="auto")
