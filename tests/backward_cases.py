"""Inputs, references, the grid arithmetic and the acceptance rule for the backward of the fused scorer (csrc/ahv_backward.hip:
the recomputing and the saved head kernel, dW1 and its reduce; csrc/ahv_bwd_volume.hip: the dV scatter; csrc/ahv_rotgrad.hip:
the head-only pass and score_rotation_grad_kernel; one head rule, csrc/ahv_bwd.h, one grid rule, backward_grid in
csrc/ahv_launch.h), shared by tests/test_backward_cases_cpu.py (the conditions the cases must meet, no GPU) and
tests/test_gpu_backward_edges.py (the kernels on every case).

What tests/fused_cases.py gives the forward, for the backward: random heads of every kind (`oc.head`), independent random
source volumes per sample, Haar rotations, grad_scores ~ N(0,1) and an UN-NORMALISED feat_tgt ~ N(0,1) per sample (what
ops._Forward3d2dFn.backward hands the kernels in production), at the hypothesis counts where `backward_grid` changes what
a workgroup does (`sizes`, `many_samples`).

Reference: oracle/torch_ref.py's op sequence under torch autograd on the CPU, in fp64 on the fp32 inputs cast up, with the
ambiguous ReLU sub-gradients fitted (backward_reference.KinkReference; KINK_TAU scaled by the case's own pre-activations:
rms of the fp64 u over 0.5, the rms of a plain case).  Yardstick: per gradient, e_ref is the error of the SAME op sequence
under autograd in fp32 on the CPU, put through KinkReference like a kernel result; a kernel passes when
e_got <= min(GRAD_RTOL, PARITY_FACTOR * e_ref).  PARITY_FACTOR = 10 is tests/test_gpu_rotation_grad.py's factor for the same
comparison (fp32 MFMA chains of 384 and float-atomic sums across hypotheses against ATen's blocked sums).  The volume
gradient is also measured per sample, each against its own largest entry, with its own e_ref: the global maximum hides a
dropped sample.  Nothing is calibrated against the kernels.

The clamp kind (b2 = 0, source volumes ~1e-13) cannot reuse the forward's scale.  fc.fused_case puts the MEDIAN column norm
on EPS, so one column is always within rounding of F.normalize's clamp, two correct evaluations take different branches
there, and the jump in the gradient -- the term c3 * v of head_tile_backward -- is as large as the term it belongs to
(fp32 against fp64 on the CPU: 8e-3 in d vol at B = 3, N = 40).  Here each source sample is scaled so that EPS is the
geometric midpoint of the WIDEST gap between consecutive sorted fp64 column norms among the central tenth of the sample's
N x 64 norms (`gap_scale`), and `conditions` holds the case to: (a) no fp64 norm within CLAMP_GAP = 1e-5 relative of EPS --
five times what KINK_TAU allows a pre-activation relative to its size (2e-6 of 0.5); (b) 40-60 % of a sample's columns
clamped; (c) at least 90 % of the hypotheses with columns on both sides; (d) the fp32 CPU reference's norms on the fp64
ones' side of EPS in every column.  Every kind: at most KINK_MAX ambiguous pre-activations, none in dead_relu, and (e) a d b2
that does not cancel (`chain_sd`: the saved and the recomputing backward are held to each other within SAVED_RTOL).  A case whose
seed misses a condition takes the next seed (`backward_case`); no condition is relaxed.

Yardsticks, measured on the CPU at 256 CUs (python -m tests.backward_cases prints them; YARDSTICK_RANGE is pinned by the twin).
e_ref of d vol_src, d feat_tgt, d W1, d W2, d b2 over the 25 cases:

    plain      B = 3, N = 1 ... 681         4.4 - 7.8e-7   2.1 - 4.1e-7   4.5 - 6.1e-7   4.0 - 6.1e-7   2.0e-7 - 1.9e-6
    plain      B = 1, N = 7 257 1025 2049   4.3 - 7.7e-7   2.6 - 9.6e-7   5.1 - 5.7e-7   5.1e-7 - 1.0e-6   1.7e-6  4.3e-6  3.0e-6  2.0e-6
    plain      B = 257, N = 1 9             6.1e-7         2.8e-7         5.7 - 8.0e-7   6.3 - 6.8e-7   4.3 - 4.5e-7
    no_bias    B = 3, N = 7 86 171          6.4e-7 - 1.4e-6  5.6 - 8.0e-7   5.4 - 8.7e-7   4.7 - 7.1e-7   3.9e-7 - 1.0e-6
    golden     B = 3, N = 7 171             5.3 - 5.8e-7   4.3 - 5.2e-7   5.4 - 7.0e-7   5.3 - 7.0e-7   1.9e-7 - 1.1e-6
    clamp      all five cases               6.2 - 7.4e-7   5.8 - 7.6e-7   5.1 - 7.0e-7   4.9 - 7.8e-7   2.8e-7 - 1.4e-6
    dead_relu  B = 3, N = 7 171             0              1.3 - 1.4e-7   0              0              4.4e-7 - 1.0e-6

d vol_src per sample: 4.2e-7 - 2.5e-6.  One case does not keep the seed its name gives: plain B = 1, N = 1025 takes the third
(condition (e): the d b2 of the first two cancels; with the first, e_ref of d b2 was 2.5e-5).  The cases hold 0 - 18 near-kink
pre-activations, the clamp cases 1 - 16 at KINK_TAU x 5e-13.
"""
import functools
import math
import os
import re

import torch
import torch.nn.functional as F

from . import fused_cases as fc
from . import oplevel_cases as oc
from .backward_reference import GRAD_RTOL, KINK_MAX, KINK_TAU, KinkReference, ref_scores_masked, relerr  # noqa: F401
from .fused_cases import _seed, haar
from .test_gpu_backward import SAVED_RTOL      # the bar of the saved against the recomputing backward: condition (e)
from .oplevel_cases import EPS, KINDS, head, items  # noqa: F401

CU_MI355X = oc.CU_MI355X
GRAD_NAMES = ("vol_src", "feat_tgt", "W1", "W2", "b2")
PARITY_FACTOR = 10.0     # PARITY_BAR's factor in tests/test_gpu_rotation_grad.py
CLAMP_GAP = 1e-5         # relative distance every fp64 column norm keeps from EPS: 5 x KINK_TAU, see the docstring
TYPICAL_U = 0.5          # rms pre-activation of a plain case: what KINK_TAU's "magnitude about 1" is in these units
assert math.isclose(CLAMP_GAP, 5 * KINK_TAU)

# ---- grid arithmetic -------------------------------------------------------------------------------------------------------
# hypotheses per workgroup and turn: copies of ahv_launch.h's constants (the CPU twin compares them with the header)
PER_WG = {"head": 4, "saved": 8, "w1": 4, "vol": 2, "du": 1}
SOURCE_NAMES = {"head": "kBwdHeadPerWg", "saved": "kBwdHeadSavedPerWg", "w1": "kBwdW1PerWg", "vol": "kBwdVolumePerWg",
                "du": "kBwdHeadDuPerWg"}
LAUNCH_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dahv_amd", "csrc", "ahv_launch.h")


def source_constants():
    """The five constants as ahv_launch.h states them: {kernel: int}."""
    with open(LAUNCH_H) as f:
        text = f.read()
    out = {}
    for k, name in SOURCE_NAMES.items():
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, text)
        assert m, name
        out[k] = int(m.group(1))
    return out


def grid(cu, B, N, p):
    """(gx, gy) of backward_grid (csrc/ahv_launch.h), restated: y strides the batch, x the hypotheses, no more workgroups
    along x than N has turns of p hypotheses, at least one."""
    gy = min(B, cu)
    return max(1, min(cu // gy, (N + p - 1) // p)), gy


# hypotheses a workgroup takes per turn of its walk.  The grid rule's per_workgroup for every kernel but the head-only pass of
# the rotation gradient: that one is kernel 1 with its four waves (hstep = 4 gx) on a grid sized with per_workgroup = 1, so
# "one more than gx" there is the first hypothesis on a second WAVE, and its second turn begins at 4 gx + 1 like kernel 1's.
WALK = dict(PER_WG, du=4)


def turns(cu, B, N, k):
    """(turns, hypotheses in the last turn) of kernel k: a sample's hypotheses are walked WALK[k] * gx at a time (slot s of
    workgroup x takes s * gx + x, then + WALK[k] * gx, ...)."""
    step = WALK[k] * grid(cu, B, N, PER_WG[k])[0]
    t = (N + step - 1) // step
    return t, N - (t - 1) * step


def rotgrad_walk(cu, B, N):
    """(gx, turns, hypotheses in the last turn) of score_rotation_grad_kernel (launch_score_rotation_grad): a workgroup per
    hypothesis, two per CU, no more than N."""
    gy = min(B, cu)
    gx = max(1, min((2 * cu + gy - 1) // gy, N))
    t = (N + gx - 1) // gx
    return gx, t, N - (t - 1) * gx


def xcd_residue(bid, nwg, ny):
    """xcd_residue (csrc/ahv_device.h), restated: the residue of workgroup x among the gx of its row."""
    if nwg < 16 or (ny > 1 and nwg % 8 != 0):
        return bid
    xcd, q, r = bid % 8, nwg // 8, nwg % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + bid // 8


def xcd_remap(gx, gy):
    """Which branch of xcd_residue a grid takes: 'identity' (the early return), 'even' (gx a multiple of 8: eight equal
    ranges) or 'ragged' (gx % 8 != 0, one row of workgroups: the first gx % 8 XCDs take one residue more).  Checked to be a
    permutation of the residues, and to be the identity exactly where it is called one."""
    res = [xcd_residue(x, gx, gy) for x in range(gx)]
    assert sorted(res) == list(range(gx))
    kind = "identity" if gx < 16 or (gy > 1 and gx % 8) else ("even" if gx % 8 == 0 else "ragged")
    assert (res == list(range(gx))) == (kind == "identity")
    return kind


def sizes(cu, B):
    """Named N for B samples on `cu` compute units, each checked with `grid` / `turns` to land where it is meant to."""
    gy = min(B, cu)
    G = cu // gy
    assert G >= 8, (cu, B)
    s = {"one": 1,                   # gx = 1 for every p
         "partial": 7,               # head gx = 2 with three of four waves in the second workgroup; saved gx = 1, 7 of 8; dV gx = 4
         "du_turn": G + 1,           # one hypothesis more than the p = 1 grid has workgroups: the head-only pass' first second wave
         "vol_turn": 2 * G + 1,      # one hypothesis into the second turn of the p = 2 kernel (dV)
         "head_turn": 4 * G + 1,     # ... of the p = 4 kernels (head, dW1) and of the head-only pass
         "all_exact": 8 * G,         # whole turns for every kernel
         "all_ragged": 8 * G + 1}    # a last turn of one hypothesis for every kernel at once
    P = PER_WG
    g = lambda k, name: grid(cu, B, s[name], P[k])
    t = lambda k, name: turns(cu, B, s[name], k)
    assert all(g(k, "one") == (1, gy) for k in P)
    assert g("head", "partial") == (2, gy) and g("w1", "partial") == (2, gy) and g("saved", "partial") == (1, gy)
    assert g("vol", "partial") == (4, gy) and g("du", "partial") == (7, gy) and all(t(k, "partial")[0] == 1 for k in P)
    assert [h for h in range(7) if h % 2 == 1] == [1, 3, 5]     # head, workgroup 1 of 2: slots 0..2 busy, slot 3 idle
    assert g("du", "du_turn") == (G, gy) and s["du_turn"] - G == 1 and all(t(k, "du_turn")[0] == 1 for k in P)
    assert g("vol", "vol_turn") == (G, gy) and t("vol", "vol_turn") == (2, 1)
    assert all(t(k, "vol_turn")[0] == 1 for k in ("head", "saved", "w1", "du"))
    if gy == 1 and G >= 64:          # one row of workgroups: du_turn gives kernel 1 and dW1 a gx that is no multiple of 8
        assert xcd_remap(g("head", "du_turn")[0], 1) == "ragged" and xcd_remap(G, 1) == ("ragged" if G % 8 else "even")
    for k in ("head", "w1", "du"):
        assert g(k, "head_turn") == (G, gy) and t(k, "head_turn") == (2, 1)
    assert t("saved", "head_turn")[0] == 1 and t("vol", "head_turn") == (3, 1)
    for k in P:
        assert g(k, "all_exact") == (G, gy) and t(k, "all_exact") == (8 // WALK[k], WALK[k] * G)
        assert g(k, "all_ragged") == (G, gy) and t(k, "all_ragged") == (8 // WALK[k] + 1, 1)
    return s


def many_samples(cu):
    """(B, (N, ...)): one sample more than there are compute units, so gx = 1 for every kernel and workgroup row 0 walks
    samples 0 and cu (re-staging volume, target fragments and d feat_tgt between them); N = 9 gives the saved head a second
    turn of one hypothesis and the recomputing head a third."""
    B, Ns = cu + 1, (1, 9)
    for n in Ns:
        assert all(grid(cu, B, n, p) == (1, cu) for p in PER_WG.values())
    assert turns(cu, B, 9, "saved") == (2, 1) and turns(cu, B, 9, "head") == (3, 1) and turns(cu, B, 9, "vol") == (5, 1)
    assert list(range(0, B, cu)) == [0, cu]
    return B, Ns


# ---- cases -----------------------------------------------------------------------------------------------------------------
def gap_scale(norms):
    """Per sample, the factor that puts EPS at the geometric midpoint of the widest gap between consecutive sorted column
    norms among the central tenth of the sample's norms (B,N,64) -> (B,)."""
    out = []
    for nb in norms.reshape(norms.shape[0], -1).double():
        s = nb.sort().values
        lo, hi = int(0.45 * s.numel()), int(math.ceil(0.55 * s.numel()))
        c = s[lo:hi]
        assert c.numel() >= 2
        k = int((c[1:] / c[:-1]).argmax())
        out.append(EPS / math.sqrt(float(c[k]) * float(c[k + 1])))
    return torch.tensor(out, dtype=torch.float64)


def column_norms(us, W2, b2):
    """Norms (B,N,64) of the columns v = W2 relu(u) + b2 before they are normalised, in the dtype of the pre-activations
    `us` (what ref_scores_masked returns beside the scores): F.normalize's own norm."""
    return torch.stack([F.conv2d(F.relu(u), W2.to(u.dtype).reshape(32, 32, 1, 1), b2.to(u.dtype)).norm(dim=1).flatten(1) for u in us])


def per_sample_err(got, ref):
    """max over samples of max|got - ref| / max|ref| within the sample (a global maximum hides a dropped sample)."""
    d = (got.double() - ref.reshape(got.shape)).flatten(1).abs().max(dim=1).values
    return float((d / ref.reshape(got.shape).flatten(1).abs().max(dim=1).values.clamp_min(1e-30)).max())


class HypothesisKinkReference(KinkReference):
    """KinkReference whose flips are evaluated on the one hypothesis they belong to: the gradients are sums over samples and
    hypotheses, and a pre-activation of hypothesis n of sample b enters no other term, so the change of the five gradients
    is that of the sub-problem (b, n) -- one hypothesis' backward per flip, not the case's (B = 257, N = 9 with 16 near-kink
    pre-activations: 29 s of reference with the base class, 4 s with this one)."""

    def _hypothesis_grads(self, b, n, flip):
        vs, ft, R, W1, W2, b2, gs = self.args
        leaves = [x.double().requires_grad_(True) for x in (vs[b:b + 1], ft[b:b + 1], W1, W2, b2)]
        Rn = (R[b] if R.dim() == 4 else R)[n:n + 1].double()
        s, _ = ref_scores_masked(leaves[0], leaves[1], Rn, leaves[2], leaves[3], leaves[4], flip)
        return torch.autograd.grad(s, leaves, grad_outputs=gs[b:b + 1, n:n + 1].double())

    def delta(self, b, idx):
        n = idx[0]
        flip = torch.zeros_like(self.us[b][n:n + 1], dtype=torch.bool)
        flip[(0,) + tuple(idx[1:])] = True
        d = [x - y for x, y in zip(self._hypothesis_grads(b, n, [flip]), self._hypothesis_grads(b, n, None))]
        out = [torch.zeros_like(self.base[0]), torch.zeros_like(self.base[1]), d[2], d[3], d[4]]
        out[0][b], out[1][b] = d[0][0], d[1][0]
        return out


class BackwardCase:
    """Inputs of one case (CPU, fp32) with its references: `ref`, the HypothesisKinkReference (fp64 gradients `ref.base`, fp64
    pre-activations `ref.us`, `scale`); `g32`, the fp32 CPU autograd gradients; `e_ref` (five, by GRAD_NAMES) and
    `e_ref_per_sample` (d vol_src sample by sample); `norm64` / `norm32`, the column norms (B,N,64) of both references."""

    def __init__(self, name, kind, seed, vs, ft, R, hd, gs):
        self.name, self.kind, self.seed, self.vs, self.ft, self.R, self.hd, self.gs = name, kind, seed, vs, ft, R, hd, gs
        self.B, self.N = vs.shape[0], R.shape[-3]
        self.args = (vs, ft, R) + tuple(hd) + (gs,)
        self.ref = HypothesisKinkReference(*self.args)
        self.u_rms = math.sqrt(sum(float((u * u).sum()) for u in self.ref.us) / sum(u.numel() for u in self.ref.us))
        self.scale = self.u_rms / TYPICAL_U
        self.ref.rescale(self.scale)
        leaves = [x.clone().requires_grad_(True) for x in (vs, ft) + tuple(hd)]
        s32, us32 = ref_scores_masked(leaves[0], leaves[1], R, *leaves[2:])
        self.g32 = [g.detach() for g in torch.autograd.grad(s32, leaves, grad_outputs=gs)]
        self.norm64, self.norm32 = column_norms(self.ref.us, hd[1], hd[2]), column_norms(us32, hd[1], hd[2])
        if len(self.ref.amb) > KINK_MAX:         # `conditions` refuses the case; no yardstick is needed
            self.e_ref, self.e_ref_per_sample, self.kinks32 = None, None, None
            return
        fit, _, self.kinks32 = self.ref.fit(self.g32, bars=[0.0] * 5)    # always fitted: e_ref is the bar's only source
        self.e_ref = [relerr(a, r.reshape(a.shape)) for a, r in zip(self.g32, fit)]
        self.e_ref_per_sample = per_sample_err(self.g32[0], fit[0])

    def bars(self):
        """(the five bars, the per-sample bar of d vol_src): min(GRAD_RTOL, PARITY_FACTOR * e_ref)."""
        return [min(GRAD_RTOL, PARITY_FACTOR * e) for e in self.e_ref], min(GRAD_RTOL, PARITY_FACTOR * self.e_ref_per_sample)

    def clamped(self):
        return self.norm64 < EPS

    def rotations(self, b):
        return self.R if self.R.dim() == 3 else self.R[b]


def conditions(case):
    """What the case misses of what the docstring asks of it: a list of strings, empty when it may be used."""
    bad = []
    n_amb = len(case.ref.amb)
    if n_amb > (0 if case.kind == "dead_relu" else KINK_MAX):
        bad.append("%d ambiguous pre-activations" % n_amb)
    if case.kind == "clamp":
        gap = float((case.norm64 / EPS - 1).abs().min())
        if gap < CLAMP_GAP:
            bad.append("(a) a column norm within %.2e of EPS" % gap)
        share = case.clamped().double().mean(dim=(1, 2))
        if share.min() < 0.4 or share.max() > 0.6:
            bad.append("(b) clamped share per sample %.3f .. %.3f" % (share.min(), share.max()))
        per_hyp = case.clamped().double().mean(dim=2)
        both = float(((per_hyp > 0) & (per_hyp < 1)).double().mean())
        if both < 0.9:
            bad.append("(c) %.3f of the hypotheses have columns on both sides" % both)
        if not torch.equal(case.norm32 < EPS, case.clamped()):
            bad.append("(d) the fp32 reference clamps other columns")
    spread = DB2_Z * math.sqrt(2.0) * chain_sd(case)[4]
    if spread > SAVED_RTOL:
        bad.append("(e) d b2 cancels: %g standard deviations between two chain evaluations are %.2e of its largest entry" % (DB2_Z, spread))
    return bad


SEED_STEPS = 8
DB2_Z = 3.0                      # condition (e), see chain_sd
YARDSTICK_RANGE = (5e-8, 1e-5)   # every non-zero e_ref of all_cases(256): the docstring's table, a factor of two either side (the
                                 # fp32 CPU reference's rounding follows the machine's threads and BLAS)


def _inputs(kind, B, N, per_sample, seed):
    hd = head(seed % 100003, kind)
    vs = items(B, seed + 1, "dead_relu" if kind == "dead_relu" else "plain")
    ft = torch.randn(B, 32, 64, generator=oc._gen(seed + 2))
    R = haar(B * N, seed + 3).reshape(B, N, 3, 3) if per_sample else haar(N, seed + 3)
    gs = torch.randn(B, N, generator=oc._gen(seed + 4))
    if kind == "clamp":
        scale = gap_scale(fc.source_column_norms(vs, R, hd))          # the norms at scale 1, as fused_case reads them
        vs = (vs.double() * scale.reshape(B, 1, 1, 1, 1)).float()
    return vs, ft, R, hd, gs


@functools.lru_cache(maxsize=None)
def backward_case(kind, B, N, per_sample):
    """The case of head `kind` with B samples and N hypotheses, R per sample (B,N,3,3) or shared (N,3,3).  Every seed follows
    from the case's name: the first of seed, seed + 16, ... whose case meets `conditions`."""
    name = "backward %s B=%d N=%d %s R" % (kind, B, N, "per-sample" if per_sample else "shared")
    missed = []
    for k in range(SEED_STEPS):
        seed = _seed(name) + 16 * k
        vs, ft, R, hd, gs = _inputs(kind, B, N, per_sample, seed)
        case = BackwardCase(name, kind, seed, vs, ft, R, hd, gs)
        case.seed_steps = k
        bad = conditions(case)
        if not bad:
            return case
        missed.append(bad)
    raise AssertionError("%s: no seed in %d meets the conditions: %s" % (name, SEED_STEPS, missed))


# ---- the rule --------------------------------------------------------------------------------------------------------------
def accept_grads(got, case, what):
    """The five gradients of a kernel against the case's bars; prints e_got, e_ref and e_got / e_ref per gradient first
    (a run with -s records them) and returns the ratios (vol_src per sample last; 0 / 0 counts as 0)."""
    got = [g.detach().cpu() for g in got]
    for g, r, name in zip(got, case.ref.base, GRAD_NAMES):
        assert g.numel() == r.numel(), (what, name)
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), "%s: d %s is not finite" % (what, name)
    bars, bar_ps = case.bars()
    fit, n_amb, flipped = case.ref.fit(got, bars)
    errs = [relerr(a, r.reshape(a.shape)) for a, r in zip(got, fit)]
    e_ps = per_sample_err(got[0], fit[0])
    ratio = lambda e, r: e / r if r > 0 else (0.0 if e == 0 else float("inf"))
    ratios = [ratio(e, r) for e, r in zip(errs, case.e_ref)] + [ratio(e_ps, case.e_ref_per_sample)]
    print("%-66s %s  per-sample vol %.2f   (e_ref %s; %d near-kink, %d flipped)" % (
        what, " ".join("%s %.2f" % (n, x) for n, x in zip(GRAD_NAMES, ratios)), ratios[5],
        " ".join("%.1e" % e for e in case.e_ref), n_amb, flipped))
    missed = ["d %s e_got %.3e above the bar %.3e (e_ref %.3e)" % (name, e, b, r)
              for name, e, b, r in zip(GRAD_NAMES + ("vol_src per sample",), errs + [e_ps], bars + [bar_ps],
                                       case.e_ref + [case.e_ref_per_sample]) if not e <= b]
    assert not missed, "%s: %s" % (what, "; ".join(missed))
    return ratios


def chain_sd(case):
    """A diagnostic, and the source of condition (e); no bar contains it.  For the two gradients that the head kernels sum
    over hypotheses with float atomics into single words -- d feat_tgt (per sample: N hypotheses) and d b2 (B N hypotheses) --
    the standard deviation of ONE fp32 accumulator's running error at the worst element, relative to the gradient's largest
    entry, in fp64 from the reference's own terms: oc.adjoint_chain_allowance's model.  Five numbers by GRAD_NAMES, zero for
    the other three.

    A wave sums a hypothesis' contribution in registers -- for d feat_tgt[b] the term g[b, n] f[b, n] / 64 (f: the normalised
    source features), for d b2[o] the sum P[b, n, o] over the 64 positions of dL/dv -- and the hypotheses' terms meet in one
    word by float atomics, in the hardware's order (several hypotheses of a wave first: fewer and larger adds than modelled
    here, never more).  For a chain of n adds in random order with sum S and sum of squares T2 the running error has standard
    deviation U32 sqrt(n (S^2 / 3 + T2 / 6) / 3) (derived in oc.adjoint_chain_allowance).

    Condition (e): the saved and the recomputing backward are two such evaluations of d b2, and the GPU file holds them to
    each other within SAVED_RTOL.  Where d b2 cancels -- the seed the name "backward plain B=1 N=1025 shared R" gives: 65 600
    terms, one standard deviation 3.4e-6 of max|d b2| against 4e-8 ... 1.0e-6 in every other case, the fp32 CPU reference itself
    2.5e-5 from fp64 -- the two differed by 3.4e-6, 4.7e-6 and 5.4e-6 in three runs of the same code, either side of
    SAVED_RTOL = 5e-6: the hardware's order of the atomics decided.  Such a case is ill-posed for that check as a clamp case
    with a norm on EPS is for its own, and takes the next seed: DB2_Z = 3 standard deviations of the difference of two
    evaluations (sqrt 2 of one) must fit inside SAVED_RTOL."""
    if not hasattr(case, "_chain"):
        W2, b2 = case.hd[1].double(), case.hd[2].double()
        sd = lambda n, S, T2: oc.U32 * (n * (S * S / 3.0 + T2 / 6.0) / 3.0).sqrt()
        P, sd_ft = [], []
        for b, u in enumerate(case.ref.us):
            with torch.enable_grad():
                v = F.conv2d(F.relu(u), W2.reshape(32, 32, 1, 1), b2).requires_grad_(True)
                f = F.normalize(v, p=2, dim=1).flatten(2)                                     # (N, 32, 64)
                s = (f * case.ft[b].double()[None]).sum(dim=1).mean(dim=-1)
                (g,) = torch.autograd.grad(s, v, grad_outputs=case.gs[b].double())
            P.append(g.flatten(2).sum(dim=-1))                                               # (N, 32)
            t = f.detach() * (case.gs[b].double() / 64.0)[:, None, None]
            assert (t.sum(dim=0) - case.ref.base[1][b]).abs().max() <= 1e-12 * t.abs().sum(dim=0).max(), "not the reference's terms"
            sd_ft.append(sd(case.N, t.sum(dim=0), (t * t).sum(dim=0)).max())
        P = torch.stack(P)
        S, T2 = P.sum(dim=(0, 1)), (P * P).sum(dim=(0, 1))
        assert (S - case.ref.base[4]).abs().max() <= 1e-12 * P.abs().sum(dim=(0, 1)).max(), "not the reference's terms"
        case._chain = [0.0, float(max(sd_ft) / case.ref.base[1].abs().max()), 0.0, 0.0,
                       float(sd(case.B * case.N, S, T2).max() / S.abs().max())]
    return case._chain


# ---- the cases of the GPU file, by the CU count ----------------------------------------------------------------------------
GRID_B3 = ("one", "partial", "du_turn", "vol_turn", "head_turn", "all_exact", "all_ragged")
GRID_B1 = ("partial", "du_turn", "head_turn", "all_ragged")   # du_turn: see xcd_remap
KIND_SIZES = ("partial", "vol_turn")
OTHER_KINDS = ("no_bias", "dead_relu", "clamp", "golden")
# beyond du_turn: plain at head_turn, a second turn of one hypothesis in the head-only pass and a second trip of
# score_rotation_grad_kernel (no smaller case has either)
ROTGRAD = (("plain", "du_turn"), ("no_bias", "du_turn"), ("clamp", "du_turn"), ("dead_relu", "partial"), ("plain", "head_turn"))


def all_cases(cu):
    """Every (kind, B, N, per_sample) tests/test_gpu_backward_edges.py runs on a device of `cu` compute units."""
    s1, s3, s2 = sizes(cu, 1), sizes(cu, 3), sizes(cu, 2)
    Bm, Nm = many_samples(cu)
    out = [("plain", 3, s3[k], True) for k in GRID_B3] + [("plain", 1, s1[k], False) for k in GRID_B1]
    out += [("plain", Bm, n, False) for n in Nm]
    out += [(kind, 3, s3[k], True) for kind in OTHER_KINDS for k in KIND_SIZES]
    out += [("clamp", 2, s2["vol_turn"], False), ("clamp", Bm, 9, False)]
    out += [(kind, 3, s3[k], True) for kind, k in ROTGRAD if (kind, 3, s3[k], True) not in out]
    return out


if __name__ == "__main__":   # the yardsticks of every case at 256 CUs (no GPU)
    for c in all_cases(CU_MI355X):
        case = backward_case(*c)
        print("%-46s e_ref %s  per-sample %.1e  u rms %.2e  near-kink %d (fp32 flipped %d)  seed steps %d" % (
            case.name, " ".join("%.2e" % e for e in case.e_ref), case.e_ref_per_sample, case.u_rms, len(case.ref.amb),
            case.kinks32, case.seed_steps), flush=True)
