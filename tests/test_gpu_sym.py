"""Pose selection modulo a symmetry group on the GPU: ``ahv_sym_fold_f32`` / ``ahv_topk_modes_sym_f32`` through ``ops.sym_fold``,
``ops.topk_modes(symmetry=)`` and ``ops.pose_posterior(symmetry=)`` against the fp64 numpy reference (tests/sym_reference.py).

DECISIONS (which anchor, which element, which hypotheses a winner kills) are compared only where the reference's margin -- the
smaller of |t_G - tau| and the gap between the best and the second-best element -- exceeds 1e-5: an fp32 summation order moves a
trace by ~1e-6.  For the fold the share of hypotheses left out this way is ASSERTED to be at most 1 % per case; for the mode lists
the seeds were chosen on the CPU (the whole reference run needs no GPU) so that NO case is left out, and that is asserted too.

VALUES (R_out, V_out, trace) are compared against fp64 with no tolerance fixed in advance: the same composition is done in stock
fp32 torch on the same inputs, and the kernel may be at most 4 x as far from fp64 as that (the margin is for a different FMA order
on 3 x 3 products, where both sides sit at a few ulp).  That rule is asserted bare on the union of all cases' inputs, and per case
with torch's error taken as at least half an ulp (a maximum over one or five samples is not "a few ulp" but any fraction of one)."""
import numpy as np
import pytest
import torch

from . import sym_reference as sr

pytestmark = pytest.mark.gpu

EMPTY = sr.EMPTY
MARGIN = 1e-5
MAX_LEFT_OUT = 0.01


@pytest.fixture(scope="module")
def dev(ahv):
    return torch.device("cuda:0")


def make_group(ahv, name):
    Sy = ahv.rotations.Symmetry
    return {"trivial": Sy.trivial_group, "c2": lambda: Sy.cyclic(2, "Z"), "d2": lambda: Sy.dihedral(2, (1.0, 2.0, 2.0)),
            "tetra": Sy.tetrahedral, "octa": Sy.octahedral, "icosa": Sy.icosahedral, "cinf": lambda: Sy.axial((2.0, -1.0, 2.0)),
            "dinf": lambda: Sy.axial("Y", flip=True)}[name]()


def sym_np(sym):
    return sym.S.numpy(), (None if sym.axis is None else sym.axis.numpy())


def haar(ahv, n, seed):
    return ahv.rotations.haar_rotations_np(n, seed)


def fold_inputs(ahv, N, B, per_sample_R, per_sample_sym, K, group, seed, with_v=True, zero_slot=True):
    """R, the group (conjugated per sample by Haar frames where asked), K Haar anchors (slot 1 all-zero when K >= 3), V."""
    sym = make_group(ahv, group)
    if per_sample_sym:
        sym = sym.conjugate(torch.from_numpy(haar(ahv, B, seed + 3)))
    R = haar(ahv, N * (B if per_sample_R else 1), seed)
    R = R.reshape(B, N, 3, 3) if per_sample_R else R
    anchors = haar(ahv, B * K, seed + 1).reshape(B, K, 3, 3).copy()
    if zero_slot and K >= 3:
        anchors[:, 1] = 0.0
    V = (np.random.default_rng(seed + 2).standard_normal((B, N, 3)) * 0.1).astype(np.float32) if with_v else None
    return R, sym, anchors, V


def compose_torch(R, A, Sg, axis, V, dtype):
    """The fold's arithmetic in stock torch at ``dtype`` for n (hypothesis, anchor, element) triples: M = A^T R S_g, the closed
    form, Q = S_g Rot, R Q, Q^T V.  -> (R_out, V_out or None, trace)."""
    R, A, Sg = (torch.as_tensor(x).to(dtype) for x in (R, A, Sg))
    M = A.transpose(-1, -2) @ R @ Sg
    tr = M.diagonal(dim1=-2, dim2=-1).sum(-1)
    Q, t = Sg, tr
    if axis is not None:
        a = torch.as_tensor(axis).to(dtype)
        p = (a[:, None, :] @ M @ a[:, :, None])[:, 0, 0]
        c = tr - p
        s = -(a[:, 0] * (M[:, 2, 1] - M[:, 1, 2]) + a[:, 1] * (M[:, 0, 2] - M[:, 2, 0]) + a[:, 2] * (M[:, 1, 0] - M[:, 0, 1]))
        h = torch.sqrt(c * c + s * s)
        ok = h > 0
        cp, sp = torch.where(ok, c / h, torch.ones_like(h)), torch.where(ok, s / h, torch.zeros_like(h))
        Kx = torch.zeros_like(M)
        Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
        eye = torch.eye(3, dtype=dtype)
        rot = cp[:, None, None] * eye + sp[:, None, None] * Kx + (1 - cp)[:, None, None] * (a[:, :, None] * a[:, None, :])
        Q, t = Sg @ rot, p + h
    Vo = None if V is None else (Q.transpose(-1, -2) @ torch.as_tensor(V).to(dtype)[:, :, None])[:, :, 0]
    return R @ Q, Vo, t


def run_fold(ahv, dev, R, sym, anchors, V, angle, keep, inplace):
    Rt = torch.from_numpy(np.ascontiguousarray(R)).to(dev)
    Vt = None if V is None else torch.from_numpy(V).to(dev)
    out = v_out = None
    if inplace:   # (per-sample R only)
        Rt = Rt.clone()
        out, v_out = Rt, Vt
    return ahv.ops.sym_fold(Rt, sym.to(dev), torch.from_numpy(anchors).to(dev), angle, keep=keep, V=Vt, out=out, V_out=v_out)


def half_ulp(x):
    """Half a unit in the last place of the fp32 numbers of magnitude x: what no fp32 result can be held to."""
    return 2.0 ** (np.floor(np.log2(x)) - 24) if x > 0 else 0.0


def measure_fold(ahv, dev, R, sym, anchors, V, angle, keep, inplace, label):
    """One fold against the reference -> what the tests assert: the share of decisions left out, whether the others agree, whether
    the copied slots are the input's bytes, and the largest errors against fp64 of the kernel and of stock fp32 torch
    (R_out, trace, V_out) on the decided and folded set."""
    S, axis = sym_np(sym)
    B, K = anchors.shape[:2]
    N = R.shape[-3]
    want = sr.fold(R, S, axis, anchors, angle, keep, V)
    got = run_fold(ahv, dev, R, sym, anchors, V, angle, keep, inplace)
    which, elem, trace = got.which.cpu().numpy(), got.elem.cpu().numpy(), got.trace.cpu().numpy()
    Ro = got.R.cpu().numpy()
    Vo = None if V is None else got.V.cpu().numpy()
    Rin = np.broadcast_to(R, (B, N, 3, 3))
    sure = want["margin"] > MARGIN
    res = {"label": label, "left_out": 1.0 - sure.mean(), "folded": int((want["which"] >= 0).sum())}
    res["decisions"] = np.array_equal(which[sure], want["which"][sure]) and np.array_equal(elem[sure], want["elem"][sure])
    # a hypothesis no anchor took, the keep slots and the identity element: the input's bytes
    same = (which < 0) | ((elem == 0) & ~want["moved"] & sure)
    res["bytes"] = (np.array_equal(Ro[same].view(np.uint32), np.ascontiguousarray(Rin[same]).view(np.uint32))
                    and (V is None or np.array_equal(Vo[same].view(np.uint32), V[same].view(np.uint32))))
    res["untaken"] = bool(np.all(np.isnan(trace[which < 0])) and np.array_equal(elem[which < 0], which[which < 0])
                          and np.all(which[:, :keep] == -1))
    # values, on the decided and folded set
    m = sure & (want["which"] >= 0)
    res["e_kern"] = res["e_torch"] = (0.0, 0.0, 0.0)
    res["floor"] = (half_ulp(1.0), half_ulp(3.0), 0.0 if V is None else half_ulp(float(np.abs(want["V"]).max())))
    if m.any():
        b_idx = np.nonzero(m)[0]
        Sb = S[b_idx, want["elem"][m]] if S.ndim == 4 else S[want["elem"][m]]
        ab = None if axis is None else (axis[b_idx] if axis.ndim == 2 else np.broadcast_to(axis, (b_idx.size, 3)).copy())
        A = anchors[b_idx, want["which"][m]]
        R32, V32, t32 = compose_torch(Rin[m], A, Sb, ab, None if V is None else V[m], torch.float32)
        err = lambda x, ref: float(np.abs(np.asarray(x, dtype=np.float64) - ref).max())
        res["e_torch"] = (err(R32.numpy(), want["R"][m]), err(t32.numpy(), want["trace"][m]),
                          0.0 if V is None else err(V32.numpy(), want["V"][m]))
        res["e_kern"] = (err(Ro[m], want["R"][m]), err(trace[m], want["trace"][m]), 0.0 if V is None else err(Vo[m], want["V"][m]))
    print("%s: left out %.2e of %d decisions, folded %d; max error vs fp64 (R_out, trace, V_out): kernel %s, stock fp32 torch %s"
          % (label, res["left_out"], B * N, res["folded"], res["e_kern"], res["e_torch"]))
    return res


# ---- the fold --------------------------------------------------------------------------------------------------------
# (N, B, per-sample R, per-sample group, K, group, angle or None, keep, V, in place).  N = 5 / 1027 / 4099 with B = 3 and a
# per-sample R: sample 1's row starts mid-vector (9 N floats and 3 N floats are no multiples of 4) and the last lane is ragged.
FOLD_CASES = [
    (1, 1, False, False, 1, "c2", None, 0, True, False), (1, 3, True, True, 3, "dinf", 60.0, 0, False, True),
    (5, 1, False, False, 3, "octa", 60.0, 2, True, False), (5, 3, True, True, 16, "cinf", None, 2, True, True),
    (5, 3, False, True, 1, "trivial", 15.0, 0, True, False),
    (1027, 1, True, False, 3, "d2", 15.0, 0, True, True), (1027, 3, True, True, 16, "tetra", 60.0, 2, True, False),
    (1027, 3, False, False, 1, "icosa", None, 0, False, False), (1027, 3, True, False, 3, "cinf", 60.0, 0, True, True),
    (1027, 1, False, True, 16, "dinf", 15.0, 2, True, False), (1027, 3, True, True, 3, "trivial", None, 0, True, False),
    (4099, 1, False, False, 3, "c2", 15.0, 0, True, False), (4099, 3, True, True, 3, "octa", None, 2, True, True),
    (4099, 3, False, True, 16, "d2", 60.0, 0, False, False), (4099, 1, True, False, 1, "tetra", 15.0, 2, True, True),
    (4099, 3, True, False, 16, "icosa", 15.0, 0, True, False), (4099, 3, True, True, 1, "dinf", None, 0, True, True),
    (4099, 1, False, False, 3, "cinf", 15.0, 0, False, False), (4099, 3, False, False, 3, "octa", 60.0, 2, True, False),
]


@pytest.fixture(scope="module")
def fold_results(ahv, dev):
    """Every case of FOLD_CASES, run once (reference and kernel) and shared by the tests below."""
    out = {}
    for case in FOLD_CASES:
        N, B, per_R, per_sym, K, group, angle, keep, with_v, inplace = case
        R, sym, anchors, V = fold_inputs(ahv, N, B, per_R, per_sym, K, group, seed=11 + N + K, with_v=with_v)
        out[case] = measure_fold(ahv, dev, R, sym, anchors, V, angle, min(keep, N), inplace and per_R,
                                 "fold N=%d B=%d K=%d %s" % (N, B, K, group))
    return out


@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_fold_against_the_reference(fold_results, case):
    """Per case: at most 1 % of the decisions left out, the others equal, the copied slots byte for byte, and the values within
    4 x stock fp32 torch's own error -- where that error is at least half an ulp of the quantity (2^-25 for an entry of R_out,
    2^-23 for a trace up to 3): the maximum over a handful of samples can be any fraction of an ulp (case N = 1, ONE hypothesis:
    torch's trace is 9.9e-9 from fp64 and the kernel's 5.0e-8, both under a quarter ulp), and no fp32 result can be held to
    less than half an ulp.  test_fold_values_over_all_cases applies the bare 4 x rule to the union of the inputs."""
    r = fold_results[case]
    assert r["left_out"] <= MAX_LEFT_OUT
    assert r["decisions"] and r["bytes"] and r["untaken"]
    for k, t, floor in zip(r["e_kern"], r["e_torch"], r["floor"]):
        assert k <= 4.0 * max(t, floor)


def test_fold_values_over_all_cases(fold_results):
    """R_out, trace and V_out against fp64 on the union of the cases' inputs: the kernel is at most 4 x as far as stock fp32 torch."""
    kern = np.max([r["e_kern"] for r in fold_results.values()], axis=0)
    stock = np.max([r["e_torch"] for r in fold_results.values()], axis=0)
    print("fold, all cases: max error vs fp64 (R_out, trace, V_out): kernel %s, stock fp32 torch %s" % (kern, stock))
    assert sum(r["folded"] for r in fold_results.values()) > 50_000 and np.all(stock > 0)
    assert np.all(kern <= 4.0 * stock)


def test_fold_in_place_equals_out_of_place_and_repeats(ahv, dev):
    """Two calls give the same bytes; in place gives the bytes of out of place."""
    R, sym, anchors, V = fold_inputs(ahv, 1027, 3, True, True, 3, "dinf", seed=5)
    a = run_fold(ahv, dev, R, sym, anchors, V, 60.0, 2, False)
    b = run_fold(ahv, dev, R, sym, anchors, V, 60.0, 2, False)
    c = run_fold(ahv, dev, R, sym, anchors, V, 60.0, 2, True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert int((a.which >= 0).sum()) > 100


def test_fold_nan_matrices_and_empty_anchors(ahv, dev):
    """A NaN matrix among R and a NaN anchor: which = -1 and the bytes are copied; an all-zero anchor list folds nothing."""
    R, sym, anchors, V = fold_inputs(ahv, 1027, 3, True, False, 3, "octa", seed=7)
    R = R.copy()
    R[1, 77, 1, 2] = np.nan
    R[2, 1026] = np.nan
    anchors[2, 0] = np.nan     # sample 2: slot 0 NaN (used, matches nothing), slot 1 empty, slot 2 takes everything
    got = run_fold(ahv, dev, R, sym, anchors, V, None, 0, False)
    which = got.which.cpu().numpy()
    assert which[1, 77] == -1 and which[2, 1026] == -1
    assert np.all(which[2, :1026] == 2) and np.all(which[0] == 0) and np.all(np.delete(which[1], 77) == 0)
    Ro = got.R.cpu().numpy()
    assert np.array_equal(Ro[1, 77].view(np.uint32), R[1, 77].view(np.uint32))
    assert np.array_equal(Ro[2, 1026].view(np.uint32), R[2, 1026].view(np.uint32))
    assert np.array_equal(got.V.cpu().numpy()[1, 77].view(np.uint32), V[1, 77].view(np.uint32))
    want = sr.fold(R, *sym_np(sym), anchors, None, 0, V)
    assert np.array_equal(which, want["which"])
    none = run_fold(ahv, dev, R, sym, np.zeros_like(anchors[:, :1]), V, None, 0, False)
    assert bool((none.which == -1).all()) and np.array_equal(none.R.cpu().numpy().view(np.uint32), R.view(np.uint32))
    assert np.array_equal(none.V.cpu().numpy().view(np.uint32), V.view(np.uint32)) and bool(torch.isnan(none.trace).all())


def test_fold_on_the_cube_lattice_is_exact(ahv, dev):
    """R, anchors and the group all from the 24 cube rotations: every trace is an exact integer in fp32 and fp64 alike, so which,
    elem and R_out must equal the reference's exactly -- exact ties (several elements reach the same trace; an anchor exactly AT
    tau) included: the first maximiser and >= decide."""
    sym = ahv.rotations.Symmetry.octahedral()
    cube = sym.S.numpy()
    rng = np.random.default_rng(3)
    R = cube[rng.integers(0, 24, size=(3, 1027))]
    anchors = cube[rng.integers(0, 24, size=(3, 3))].copy()
    V = rng.integers(-3, 4, size=(3, 1027, 3)).astype(np.float32)
    ties = 0
    for group, angle in ((ahv.rotations.Symmetry.cyclic(4, "Z"), 90.0), (ahv.rotations.Symmetry.dihedral(2, "X"), 90.0),
                         (sym, None), (ahv.rotations.Symmetry.cyclic(2, "Y"), None)):
        if angle is not None:   # tau is then an exact integer trace (1 at 90 degrees): t_G == tau happens
            assert sr.tau_of(angle) == 1.0
        want = sr.fold(R, *sym_np(group), anchors, angle, 0, V)
        got = run_fold(ahv, dev, R, group, anchors, V, angle, 0, False)
        ties += int((want["margin"] == 0).sum())
        assert np.array_equal(got.which.cpu().numpy(), want["which"]) and np.array_equal(got.elem.cpu().numpy(), want["elem"])
        assert np.array_equal(got.R.cpu().numpy(), want["R"]) and np.array_equal(got.V.cpu().numpy(), want["V"])
        assert np.array_equal(got.trace.cpu().numpy(), want["trace"], equal_nan=True)
    assert ties > 100


# ---- distinct modes modulo the group ---------------------------------------------------------------------------------
# (N, B, per-sample R and group, K, group, angle, seed): the seeds were chosen on the CPU so that the reference's margin exceeds
# 1e-5 in every case (the assertion below).  K = 64 sits where N K B G decisions leave such seeds.
MODES_CASES = [
    (1, 1, False, 1, "c2", 15.0, 0), (1, 3, True, 8, "octa", 60.0, 0), (4, 1, False, 8, "dinf", 15.0, 0), (4, 3, True, 64, "icosa", 60.0, 0),
    (5, 3, True, 8, "cinf", 60.0, 0), (5, 1, False, 64, "d2", 15.0, 0), (1023, 1, False, 64, "c2", 15.0, 0),
    (1023, 3, True, 8, "tetra", 15.0, 3), (1023, 3, False, 8, "dinf", 60.0, 0), (1023, 3, True, 64, "trivial", 60.0, 0),
    (1025, 3, True, 8, "octa", 15.0, 3), (1025, 1, False, 64, "cinf", 60.0, 0), (1025, 3, False, 1, "icosa", 15.0, 0),
    (1025, 3, True, 8, "d2", 60.0, 0), (4099, 1, False, 8, "icosa", 15.0, 23), (4099, 3, True, 8, "c2", 15.0, 1),
    (4099, 3, False, 8, "cinf", 15.0, 2), (4099, 3, True, 64, "octa", 60.0, 1), (4099, 1, True, 8, "dinf", 15.0, 0),
    (4099, 3, True, 8, "tetra", 60.0, 2), (4099, 3, False, 1, "trivial", 15.0, 0),
]


def modes_inputs(ahv, N, B, per_sample, group, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, N)).astype(np.float32)
    R = haar(ahv, N * (B if per_sample else 1), seed + 1)
    sym = make_group(ahv, group)
    if per_sample:
        sym = sym.conjugate(torch.from_numpy(haar(ahv, B, seed + 2)))
    return s, (R.reshape(B, N, 3, 3) if per_sample else R), sym


def run_modes(ahv, dev, s, R, K, angle, sym, n_offset=0):
    keys = ahv.ops.topk_modes(torch.from_numpy(s).to(dev), torch.from_numpy(np.ascontiguousarray(R)).to(dev), K, angle,
                              n_offset=n_offset, symmetry=None if sym is None else sym.to(dev))
    return keys.cpu()


@pytest.mark.parametrize("N,B,per_sample,K,group,angle,seed", MODES_CASES)
def test_modes_list_equals_the_reference(ahv, dev, N, B, per_sample, K, group, angle, seed):
    s, R, sym = modes_inputs(ahv, N, B, per_sample, group, seed)
    want, margin = sr.select_modes(s, R, K, angle, *sym_np(sym), n_offset=7)
    print("modes N=%d B=%d K=%d %s: margin %.3e" % (N, B, K, group, margin))
    assert margin > MARGIN          # no case is left out
    got = run_modes(ahv, dev, s, R, K, angle, sym, n_offset=7)
    assert got.shape == (B, K) and got.dtype == torch.int64
    assert torch.equal(got, torch.from_numpy(want))
    if group == "trivial":          # the plain kernel's list, bit for bit
        assert torch.equal(got, run_modes(ahv, dev, s, R, K, angle, None, n_offset=7))


def test_trivial_group_equals_plain_modes_on_non_rotations(ahv, dev):
    """G = 1, no axis: the bytes of ``ops.topk_modes`` whatever the matrices are (scaled, zero, NaN) and whatever the scores."""
    N, K = 2050, 16
    rng = np.random.default_rng(2)
    s = (np.round(rng.standard_normal((3, N)) * 4) / 4).astype(np.float32)
    s[0, 5], s[0, 9], s[1, 3] = np.nan, np.inf, -np.inf
    R = haar(ahv, 3 * N, 4).reshape(3, N, 3, 3).copy()
    R[0, 17] = 0.0
    R[1, 100] *= 1.5
    R[2, 2049, 0, 0] = np.nan
    sym = ahv.rotations.Symmetry.trivial_group()
    assert torch.equal(run_modes(ahv, dev, s, R, K, 15.0, sym), run_modes(ahv, dev, s, R, K, 15.0, None))


def orbit_set(ahv, sym, n, seed):
    """n Haar rotations TOGETHER WITH their orbit copies R_i S_g (fp64 products rounded to fp32), every copy with its original's
    score: (scores (1, n G), R (n G, 3, 3), orbit id per entry)."""
    S = sym.S.numpy().astype(np.float64)
    G = S.shape[0]
    R0 = haar(ahv, n, seed).astype(np.float64)
    R = (R0[:, None] @ S[None]).reshape(n * G, 3, 3).astype(np.float32)
    s0 = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    return np.repeat(s0, G)[None], R, np.repeat(np.arange(n), G)


def test_one_mode_per_orbit(ahv, dev):
    """On a set made of Haar rotations and their orbit copies the symmetric list holds at most one member of any orbit; the plain
    list holds several (the copies of the best orbit are 90 degrees or more apart, far outside 15 degrees, and share the top score)."""
    sym = ahv.rotations.Symmetry.octahedral()
    s, R, orbit = orbit_set(ahv, sym, 171, seed=1)            # 4104 hypotheses
    K = 8
    want, margin = sr.select_modes(s, R, K, 15.0, *sym_np(sym))
    assert margin > MARGIN
    got = run_modes(ahv, dev, s, R, K, 15.0, sym)
    assert torch.equal(got, torch.from_numpy(want))
    o_sym = orbit[sr.indices(got.numpy())[0]]
    assert len(set(o_sym.tolist())) == K                       # K distinct orbits
    o_plain = orbit[sr.indices(run_modes(ahv, dev, s, R, K, 15.0, None).numpy())[0]]
    assert len(set(o_plain.tolist())) == 1                     # the plain list: K copies of ONE pose (24 copies share the top score)
    assert o_plain[0] == o_sym[0]


def test_modes_nan_scores_non_rotations_and_padding(ahv, dev):
    """NaN scores and a non-rotation behave as the reference restatement says; the list is padded EMPTY when the quotient runs out
    of modes (octahedral group at 60 degrees: the caps of an orbit cover most of SO(3))."""
    N, K = 1025, 64
    s, R, sym = modes_inputs(ahv, N, 3, True, "octa", seed=21)
    s, R = s.copy(), R.copy()
    s[0, 3], s[1, 1024], s[2, 500] = np.nan, np.nan, np.inf
    R[0, 10] = 0.0
    R[1, 11] *= 2.0
    want, margin = sr.select_modes(s, R, K, 60.0, *sym_np(sym))
    assert margin > MARGIN
    got = run_modes(ahv, dev, s, R, K, 60.0, sym)
    assert torch.equal(got, torch.from_numpy(want))
    g = got.numpy()
    assert (g[:, -1] == EMPTY).all() and (g[:, 0] != EMPTY).all()      # the quotient ran out before K = 64
    assert sr.indices(g)[0, 0] == 3 and sr.indices(g)[1, 0] == 1024     # NaN sorts first


# ---- the posterior modulo the group ----------------------------------------------------------------------------------

def test_posterior_sums_the_orbit(ahv, dev):
    """On a set with its orbit copies the symmetric posterior's mode masses are the SUM over each orbit of the plain call's masses,
    and its mean pose is as near the planted one as the plain call's own mean poses are near theirs; on pre-folded input it is the
    plain call bit for bit."""
    sym = ahv.rotations.Symmetry.dihedral(2, "Z")
    S = sym.S.numpy().astype(np.float64)
    G, n, ANGLE = 4, 1025, 15.0
    rng = np.random.default_rng(8)
    planted = haar(ahv, 2, 30).astype(np.float64)
    R0 = haar(ahv, n, 31).astype(np.float64)
    # half of the set sits within ~8 degrees of one of the two planted poses
    w = rng.standard_normal((n // 2, 3)) * np.radians(3.0)
    R0[: n // 2] = planted[rng.integers(0, 2, n // 2)] @ ahv.rotations.axis_angle_to_matrix(torch.from_numpy(w)).numpy()
    s0 = rng.standard_normal(n).astype(np.float32) * 0.2
    R = (R0[:, None] @ S[None]).reshape(1, n * G, 3, 3).astype(np.float32)
    s = np.repeat(s0, G)[None]
    Rt, st = torch.from_numpy(R).to(dev), torch.from_numpy(s).to(dev)
    anchors = torch.from_numpy(planted[None].astype(np.float32)).to(dev)                                   # (1,2,3,3)
    orbit_anchors = torch.from_numpy((planted[:, None] @ S[None]).reshape(1, 2 * G, 3, 3).astype(np.float32)).to(dev)
    post = ahv.ops.pose_posterior(st, Rt, 0.1, anchors=anchors, min_angle_deg=ANGLE, symmetry=sym.to(dev))
    plain = ahv.ops.pose_posterior(st, Rt, 0.1, anchors=orbit_anchors, min_angle_deg=ANGLE)
    summed = plain.mode_prob.double().reshape(1, 2, G).sum(-1)
    assert float(plain.mode_prob.min()) > 0.01 and float(summed.sum()) > 0.3
    # fp32 outputs of fp64 sums: a sum of G probabilities against one, a few ulp of 1
    assert torch.allclose(post.mode_prob.double(), summed, rtol=0, atol=G * 2.0 ** -22)
    assert abs(float(post.rest_prob) - float(plain.rest_prob)) <= G * 2.0 ** -22
    geo = lambda a, b: ahv.rotations.geodesic_deg(a.cpu().double(), b.cpu().double())
    own = float(geo(plain.mode_R_mean[0], orbit_anchors[0]).max())     # the plain call's own error
    err = float(geo(post.mode_R_mean[0], anchors[0]).max())
    print("mean pose: symmetric %.6f deg, plain call's own %.6f deg" % (err, own))
    # (a plain bucket holds the same members as the symmetric one, turned by S_g: the two errors differ by the fp32 rounding of the
    # copies and of the output matrices, ~1e-7 in Frobenius norm = ~1e-5 degrees; 1e-4 degrees of slack for it)
    assert err <= own + 1e-4
    folded = ahv.ops.sym_fold(Rt, sym.to(dev), anchors, ANGLE).R
    again = ahv.ops.pose_posterior(st, folded, 0.1, anchors=anchors, min_angle_deg=ANGLE)
    for x, y in zip(post[:10], again[:10]):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert torch.equal(post.state, again.state)


# ---- the tracker ------------------------------------------------------------------------------------------------------
TB = 3
NAMES = ("particles", "scores", "score", "idx", "R_map", "reacquired", "draws")


@pytest.fixture(scope="module")
def pair(dev):
    from .conftest import load_golden
    g, h = load_golden("batched"), load_golden("score_n128")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return T(g["vol_src"]), T(g["vol_tgt"]), tuple(T(h[k]) for k in ("W1", "W2", "b2"))


class HandFold:
    """``ops`` with ONE ``ops.sym_fold`` issued by hand after the predict step: the chain ``PoseTracker(symmetry=)`` is to issue,
    spelled out -- in place on the step's buffers, the previous ``select_rotation``'s pose as the single anchor, no limit."""

    def __init__(self, ops, sym):
        self.ops, self.sym, self.anchor = ops, sym, None

    def __getattr__(self, name):
        return getattr(self.ops, name)

    def select_rotation(self, *a, **kw):
        res = self.ops.select_rotation(*a, **kw)
        self.next_anchor = res[2]
        return res

    def diffuse_rotations(self, *a, **kw):
        R = self.ops.diffuse_rotations(*a, **kw)
        self.ops.sym_fold(R, self.sym, self.next_anchor[:, None], None, keep=1, out=R, want_info=False)
        return R

    def predict_rotations(self, *a, **kw):
        R, V = self.ops.predict_rotations(*a, **kw)
        self.ops.sym_fold(R, self.sym, self.next_anchor[:, None], None, keep=2 if kw["coast"] else 1, V=V, out=R, V_out=V,
                          want_info=False)
        return R, V


def trajectory(ahv, dev, pair, motion, steps=4, **kw):
    """[(TrackStep, velocities or None)] of ``steps`` steps after init, cloned."""
    vs, vt, w = pair
    a = dict(particles=257, sigma_deg=3.0, n_fresh=8, temperature=0.05, batch=TB, seed=1, motion=motion)
    if motion != "walk":
        a.update(sigma_vel_deg=1.0, damping=0.9)
    a.update(kw)
    t = ahv.track.PoseTracker(*w, **a)
    t.init(vs, vt, torch.from_numpy(haar(ahv, 300, 5)).to(dev))
    outs = []
    for k in range(steps):
        o = t.step(vs, (0.75 * vt + 0.25 * torch.roll(vt, k + 1, dims=0)).contiguous())
        outs.append((type(o)(*[x.clone() if isinstance(x, torch.Tensor) else x for x in o]),
                     None if t.velocities is None else t.velocities.clone()))
    return outs


def same_bytes(a, b):
    for k, ((x, vx), (y, vy)) in enumerate(zip(a, b)):
        for name in NAMES:
            p, q = getattr(x, name), getattr(y, name)
            assert torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q), (k, name)
        assert (vx is None) == (vy is None)
        if vx is not None:
            assert torch.equal(vx.view(torch.int32), vy.view(torch.int32)), k


@pytest.fixture(scope="module")
def track_sym(ahv, dev):
    return ahv.rotations.Symmetry.dihedral(2, "Z").conjugate(torch.from_numpy(haar(ahv, TB, 9))).to(dev)


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_tracker_is_the_chain_with_the_fold_inserted(ahv, dev, pair, track_sym, motion):
    got = trajectory(ahv, dev, pair, motion, symmetry=track_sym)
    hand = trajectory(ahv, dev, pair, motion, backend=HandFold(ahv.ops, track_sym))
    same_bytes(got, hand)
    plain = trajectory(ahv, dev, pair, motion)
    assert not torch.equal(got[0][0].particles, plain[0][0].particles)             # the fold moved something
    # the cloud lives in one fundamental domain around the previous MAP pose: no equivalent pose is nearer to it
    S = track_sym.S.cpu().numpy()
    for (prev, _), (cur, _) in zip(got, got[1:]):
        for b in range(TB):
            P, A = cur.particles[b, 2:].cpu().numpy(), prev.R_map[b].cpu().numpy()
            tG = sr.sym_trace(P, A, S[b])[0]
            assert np.abs(tG - np.einsum("nij,ij->n", P.astype(np.float64), A.astype(np.float64))).max() < 1e-5
        assert torch.equal(cur.particles[:, 0], prev.R_map)                        # the elite: bit for bit


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_tracker_with_the_trivial_group_is_the_plain_tracker(ahv, dev, pair, motion):
    same_bytes(trajectory(ahv, dev, pair, motion, symmetry=ahv.rotations.Symmetry.trivial_group().to(dev)),
               trajectory(ahv, dev, pair, motion))


@pytest.mark.parametrize("motion", ["walk", "constant_velocity"])
def test_tracker_captured_steps_equal_eager_steps(ahv, dev, pair, track_sym, motion):
    same_bytes(trajectory(ahv, dev, pair, motion, steps=6, symmetry=track_sym),
               trajectory(ahv, dev, pair, motion, steps=6, symmetry=track_sym, use_graph=True))
