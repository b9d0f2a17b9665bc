"""Inputs, references and the plan arithmetic for the fused scorer (csrc/ahv_score.hip with ahv_dual.h, ahv_team.h,
ahv_split.h, ahv_exact.h: score_hypotheses_dual_kernel<SPLIT, TGT>, score_hypotheses_train_kernel, coarse_to_fine_kernel),
shared by tests/test_fused_cases_cpu.py (the conditions the cases must meet, no GPU) and tests/test_gpu_fused_edges.py (every
launch plan and head regime, each score against fp64).

What tests/oplevel_cases.py gives the op level, for the fused path: every sample of a batch is independent random data on
both sides, the rotations are Haar and distinct per sample, the heads are random (`oc.head`), and the yardstick is the
reference's own: oracle/torch_ref.py's score_hypotheses on the CPU in fp64 on the fp32 inputs cast up (`ref64`) and in fp32
(`ref32`), e_ref = max|ref32 - ref64|, and a launch passes when e_got <= MARGIN * e_ref (`oc.accept`).  One class of cases has
no yardstick in e_ref -- fewer than 64 scores, or dead_relu, whose scores are all one number (`few_draws`) -- and gets
`rsq_allowance` beside it, derived in fp64 from the reference's own terms (`accept_scores`, `bar`).

Head kinds (`oc.KINDS`): plain; no_bias (b2 = 0); dead_relu (W1 <= 0 and |randn| volumes on both sides: a rotated volume is
a convex blend of non-negative voxels and zero padding, every pre-activation is <= 0, v = b2 at every position of both
sides and every score is <b2/|b2|, b2/|b2|> = 1); golden (the head of tests/golden/score_n128.npz on random volumes); clamp:
b2 = 0, target volumes at scale 1, and each SOURCE sample scaled so that the median fp64 norm of its N x 64 pre-normalised
columns is EPS = 1e-12 -- half of the hot loop's columns take the clamp branch of d * rsq(max(|v|^2, 1e-24)) and half do not,
inside almost every hypothesis.  The scale is read off the reference's own norms of the ROTATED volumes (rotation and zero
padding lower them: with oc.clamp_scale on the un-rotated items every rotated column is clamped).
"""
import functools
import importlib
import zlib

import torch

from . import oplevel_cases as oc
from .oplevel_cases import EPS, KINDS, MARGIN, accept, errors, head, inf_column_case, items, plant, ref32, ref64  # noqa: F401

CU_MI355X = oc.CU_MI355X
OLD_SCORE_RTOL, OLD_SCORE_FLOOR = 1e-4, 1e-2      # tests/test_gpu_parity.py: |got - ref| <= 1e-4 max(|ref|, 1e-2) per score


# ---- plan arithmetic -------------------------------------------------------------------------------------------------------
def plan(B, N, cu, teams):
    """(gx, gy, n_main) of plan_score_launch (csrc/ahv_score.hip), restated: a persistent grid of gx x gy workgroups of
    eight waves, gy samples at a time; hypotheses [0, n_main) of a sample go to single waves in rounds of 8 gx, the rest
    -- a remainder of at most two per workgroup -- to teams of four waves."""
    gy = min(B, cu)
    gx = max(1, min(cu // gy, (N + 1) // 2 if teams else (N + 3) // 4))
    slots = 8 * gx
    rem = N % slots
    return gx, gy, (N - rem if teams and 0 < rem <= 2 * gx else N)


def sizes(cu, B):
    """N per launch shape for B samples on `cu` compute units, each checked with `plan` to land where it is meant to."""
    G = cu // min(B, cu)
    assert G >= 4, (cu, B)
    s = {"one": 1, "pair": 2,                 # all teams, gx = 1
         "teams_odd": 7,                      # all teams, gx = 4, one of the eight team slots idle
         "teams_last": 2 * G,                 # the largest all-team launch
         "lone_first": 2 * G + 1,             # single waves only, one partial round
         "round_exact": 8 * G,                # one full round and nothing left
         "tail_team_first": 8 * G + 1,        # a round + one hypothesis by a team
         "tail_team_last": 10 * G,            # a round + the largest team tail
         "tail_lone_first": 10 * G + 1}       # a round + a tail left to lone waves
    p = lambda k: plan(B, s[k], cu, True)
    assert p("one") == (1, min(B, cu), 0) and p("pair") == (1, min(B, cu), 0)
    assert p("teams_odd") == (4, min(B, cu), 0)
    assert p("teams_last") == (G, min(B, cu), 0)
    assert p("lone_first") == (G, min(B, cu), s["lone_first"]) and s["lone_first"] < 8 * G
    assert p("round_exact") == (G, min(B, cu), 8 * G)
    assert p("tail_team_first") == (G, min(B, cu), 8 * G) and p("tail_team_last") == (G, min(B, cu), 8 * G)
    assert p("tail_lone_first") == (G, min(B, cu), s["tail_lone_first"])
    return s


def no_team_sizes(cu, B):
    """N for the launches without teams (no_teams, split-f16, the training forward): one hypothesis, fewer than a
    workgroup's eight waves, one full round, a round + 3."""
    G = cu // min(B, cu)
    s = (1, 7, 8 * G, 8 * G + 3)
    assert [plan(B, n, cu, False)[0] for n in s] == [1, 2, G, G]
    assert all(plan(B, n, cu, False)[2] == n for n in s)
    return s


def many_samples(cu):
    """(B, (N, ...)): one sample more than there are compute units, so gx = 1 everywhere and one workgroup loops over two
    samples; the three N are all teams, lone waves only, and a round + a team."""
    B, Ns = cu + 1, (2, 5, 9)
    assert [plan(B, n, cu, True) for n in Ns] == [(1, cu, 0), (1, cu, 5), (1, cu, 8)]
    return B, Ns


def c2f_sizes(cu, B=2):
    """(N, N2) of the coarse-to-fine cases: stage 0 is a round + one hypothesis by a team; stage 1 runs on stage 0's grid
    (launch_coarse_to_fine's n_main2 rule) and has a round + a team tail of three there."""
    G = cu // min(B, cu)
    N, N2 = sizes(cu, B)["tail_team_first"], 8 * G + 3
    gx = plan(B, N, cu, True)[0]
    assert gx == G and 0 < N2 % (8 * gx) <= 2 * gx and gx * min(B, cu) <= cu
    return N, N2


def c2f_plan(B, N, N2, cu, teams=True):
    """(gx, gy, n_main, n_main2) of launch_coarse_to_fine."""
    gx, gy, n_main = plan(B, N, cu, teams)
    rem2 = N2 % (8 * gx)
    return gx, gy, n_main, (N2 - rem2 if teams and 0 < rem2 <= 2 * gx else N2)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _seed(name):
    return zlib.crc32(name.encode())


def haar(n, seed):
    return torch.from_numpy(importlib.import_module("3dahv_amd.rotations").haar_rotations_np(n, seed % (1 << 31)))


def source_column_norms(vol_src, R, hd):
    """fp64 norms (B,N,64) of the columns of forward_3d2d(rotate_volume(vol_src[b], R[b])) BEFORE they are normalised, for
    a head with b2 = 0, read off the reference itself: on a probe small enough that every column is clamped the output's
    norm is |v| / EPS, and the head is positively homogeneous."""
    assert not hd[2].any()
    B = vol_src.shape[0]
    probe = 1e-14
    out = []
    for b in range(B):
        Rb = (R if R.dim() == 3 else R[b]).double()
        rows = []
        for n0 in range(0, Rb.shape[0], 256):
            Rc = Rb[n0:n0 + 256]
            rot = ref64("rotate_volume", vol_src[b:b + 1].double() * probe, Rc)
            f = ref64("forward_3d2d", rot, *hd).norm(dim=1)
            assert float(f.max()) < 0.5, "probe not clamped"
            rows.append(f * (EPS / probe))
        out.append(torch.cat(rows))
    return torch.stack(out)


class FusedCase:
    """Inputs of one launch with its references (all on the CPU): scores r32 / r64 (B,N), target features ft32 / ft64
    (B,32,64); clamp cases carry the fp64 norms of their source columns, src_norm (B,N,64)."""

    def __init__(self, name, kind, vol_src, vol_tgt, R, hd, src_norm=None):
        self.name, self.kind, self.vol_src, self.vol_tgt, self.R, self.hd, self.src_norm = name, kind, vol_src, vol_tgt, R, hd, src_norm
        self.B, self.N = vol_src.shape[0], R.shape[-3]
        args = (vol_src, vol_tgt, R) + tuple(hd)
        self.r32, self.r64 = ref32("score_hypotheses", *args), ref64("score_hypotheses", *args)
        self.ft32, self.ft64 = ref32("forward_3d2d", vol_tgt, *hd), ref64("forward_3d2d", vol_tgt, *hd)

    def e_ref(self):
        return errors(self.r32, self.r32, self.r64)[1]


def _dead_relu_head(seed):
    """With both sides dead every score is |b2 / |b2||^2, and its fp32 evaluation is often the fp32 number nearest to fp64's
    (1.0 against 1.0 or 1 - 2e-16): e_ref is then zero or fp64's epsilon, no yardstick of an fp32 evaluation.  The head is the
    first of the seeds seed, seed + 1, ... whose fp32 reference is NOT the correctly rounded fp64 one (e_ref >= 2^-25, half
    an ulp below 1) -- a condition on the reference alone (the score depends on neither the volumes nor R, so one
    hypothesis shows it)."""
    vol, R = items(1, 1, "dead_relu"), haar(1, 1)
    for s in range(seed, seed + 64):
        hd = head(s, "dead_relu")
        args = (vol, vol, R) + tuple(hd)
        if errors(ref32("score_hypotheses", *args), ref32("score_hypotheses", *args), ref64("score_hypotheses", *args))[1] >= 2.0 ** -25:
            return hd
    raise AssertionError("no dead_relu head with a yardstick from seed %d on" % seed)


def _inputs(name, kind, B, N, per_sample):
    seed = _seed(name)
    hd = _dead_relu_head(seed % 100003) if kind == "dead_relu" else head(seed % 100003, kind)
    vol_src = items(B, seed + 1, "dead_relu" if kind == "dead_relu" else "plain")
    vol_tgt = items(B, seed + 2, "dead_relu" if kind == "dead_relu" else "plain")
    R = haar(B * N, seed + 3).reshape(B, N, 3, 3) if per_sample else haar(N, seed + 3)
    return hd, vol_src, vol_tgt, R


@functools.lru_cache(maxsize=None)
def fused_case(kind, B, N, per_sample):
    """The case of head `kind` with B samples and N hypotheses, R per sample (B,N,3,3) or shared (N,3,3); every seed
    follows from the case's name."""
    name = "fused %s B=%d N=%d %s R" % (kind, B, N, "per-sample" if per_sample else "shared")
    hd, vol_src, vol_tgt, R = _inputs(name, kind, B, N, per_sample)
    src_norm = None
    if kind == "clamp":
        norms = source_column_norms(vol_src, R, hd)                      # at scale 1
        scale = EPS / norms.reshape(B, -1).median(dim=1).values          # per sample
        vol_src = (vol_src.double() * scale.reshape(B, 1, 1, 1, 1)).float()
        src_norm = norms * scale.reshape(B, 1, 1)
    return FusedCase(name, kind, vol_src, vol_tgt, R, hd, src_norm)


@functools.lru_cache(maxsize=None)
def c2f_case(kind, B, N, N2):
    """A coarse-to-fine case: fused_case(kind, B, N, per-sample R) with N2 Haar refinements D shared by the batch."""
    case = fused_case(kind, B, N, True)
    return case, haar(N2, _seed(case.name + " D N2=%d" % N2))


def fine_refs(case, D, coarse_idx):
    """(ref32, ref64) of stage 1's scores (B,N2) at R[b, coarse_idx[b]] @ D, composed in fp32 for ref32 and in fp64 for ref64."""
    out = []
    for dt, ref in ((torch.float32, ref32), (torch.float64, ref64)):
        Rf = torch.stack([case.R[b, int(coarse_idx[b])].to(dt) @ D.to(dt) for b in range(case.B)])
        out.append(ref("score_hypotheses", case.vol_src, case.vol_tgt, Rf, *case.hd))
    return out


class NanNormCase:
    """oc.inf_column_case(3) as the target side of a batch of three: the middle sample's target volume holds one +inf voxel
    that puts +-inf beside NaN into one column before it is normalised (its norm is NaN).  vol_tgt is the planted batch,
    vol_tgt_clean the same without the voxel; ft32 / ft64 are the references of the planted batch."""

    def __init__(self, N):
        self.name = "fused inf-column target B=3 N=%d" % N
        clean, bad, m, hd, _, _ = inf_column_case(3)
        assert m == 1
        seed = _seed(self.name)
        self.B, self.N, self.flagged, self.hd = 3, N, m, hd
        self.vol_tgt_clean, self.vol_tgt = clean, bad
        self.vol_src = items(3, seed + 1)
        self.R = haar(3 * N, seed + 3).reshape(3, N, 3, 3)
        args = (self.vol_src, bad, self.R) + tuple(hd)
        self.r32, self.r64 = ref32("score_hypotheses", *args), ref64("score_hypotheses", *args)
        self.ft32, self.ft64 = ref32("forward_3d2d", bad, *hd), ref64("forward_3d2d", bad, *hd)


@functools.lru_cache(maxsize=None)
def nan_norm_case(N):
    return NanNormCase(N)


# ---- rules -----------------------------------------------------------------------------------------------------------------
def assert_not_weaker(case):
    """The bar (MARGIN * e_ref, with the few-draw cases' allowance) is never looser than the old per-score bar
    1e-4 max(|ref|, 1e-2), taken at its tightest element."""
    old = float((OLD_SCORE_RTOL * case.r64.abs().clamp_min(OLD_SCORE_FLOOR)).min())
    assert bar(case)[0] <= old, "%s: %g x e_ref + allowance = %.3e is looser than the old bar %.3e" % (
        case.name, MARGIN, bar(case)[0], old)


RSQ_ULP = 2.0 ** -23     # v_rsq_f32 is good to 1 ulp; an ulp is up to 2^-23 of the value
FEW_DRAWS = 64


def few_draws(case):
    """e_ref over n scores is the largest of n draws of the reference's rounding error.  MARGIN's second factor of two --
    the spread between the maxima of two independent error samples of one size -- is a statement about maxima over many
    draws; ONE draw lies below a quarter of its own standard deviation one time in five, and then no fp32 evaluation in
    another order is within 4 e_ref.  The cases with fewer than FEW_DRAWS scores are such, and so is every dead_relu case:
    all its scores are one number."""
    return case.B * case.N < FEW_DRAWS or case.kind == "dead_relu"


def rsq_allowance(case):
    """What a 1-ulp reciprocal square root per position may cost a score, in fp64 from the reference's own quantities.

    The scorer normalises a source column as d_p * rsq(max(|v_p|^2, 1e-24)) (hyp_score_tail, team_tile_score): v_rsq_f32, 1
    ulp, where the reference divides by a correctly rounded sqrt.  Position p's term c_p = <f_src_p, f_tgt_p> moves by at most
    RSQ_ULP |c_p|, and the score, their mean over the 64 positions, by at most RSQ_ULP mean_p |c_p| if all 64 err one way.
    Returned: the largest such bound over the B N scores of the case."""
    worst = 0.0
    for b in range(case.B):
        Rb = (case.R if case.R.dim() == 3 else case.R[b])
        for n0 in range(0, Rb.shape[0], 256):
            rot = ref64("rotate_volume", case.vol_src[b:b + 1], Rb[n0:n0 + 256])
            c = (ref64("forward_3d2d", rot, *case.hd) * case.ft64[b][None]).sum(1)          # (n, 64)
            assert ((c.mean(-1) - case.r64[b, n0:n0 + 256]).abs() <= 1e-12).all(), "not the reference's terms"
            worst = max(worst, float(c.abs().mean(-1).max()))
    return RSQ_ULP * worst


def bar(case):
    """(MARGIN * e_ref + allowance, allowance): the allowance is rsq_allowance for the few-draw cases and zero otherwise."""
    if not hasattr(case, "_bar"):
        A = rsq_allowance(case) if few_draws(case) else 0.0
        case._bar = (MARGIN * case.e_ref() + A, A)
    return case._bar


def accept_scores(got, case, what):
    """oc.accept for the scores of a case: e_got <= MARGIN * e_ref, plus rsq_allowance where few_draws(case)."""
    e_got, e_ref = errors(got, case.r32, case.r64)
    assert e_ref > 0.0, what + ": fp32 reference equals fp64, no yardstick"
    limit, A = bar(case)
    print("%-74s e_got %.3e  e_ref %.3e  e_got/e_ref %.2f%s" % (
        what, e_got, e_ref, e_got / e_ref, "  (few draws: + %.3e, e_got/bar %.2f)" % (A, e_got / limit) if A else ""))
    assert e_got <= limit, "%s: e_got %.3e above %g x e_ref %.3e + %.3e (ratio %.2f)" % (what, e_got, MARGIN, e_ref, A, e_got / e_ref)
    return e_got / e_ref


def clamp_shares(case):
    """(share of clamped columns per sample (B,), per hypothesis (B,N)) of a clamp case, by the fp64 norms."""
    clamped = (case.src_norm < EPS).double()
    return clamped.mean(dim=(1, 2)), clamped.mean(dim=2)


def check_key(scores, best, idx, r64, limit, what):
    """The packed key against the launch's own scores -- torch.max: the exact fp32 value, the first maximal index -- and
    its index against the fp64 arg-max wherever the fp64 top two differ by more than 2 * limit, `limit` being the bar the
    scores are under (MARGIN * e_ref; bar(case)[0] for the few-draw cases)."""
    scores, best, idx = scores.detach().cpu(), best.detach().cpu(), idx.detach().cpu()
    want, want_idx = torch.max(scores, dim=1)
    assert torch.equal(best, want) and torch.equal(idx, want_idx), "%s: the key is not torch.max of the launch's scores" % what
    if r64.shape[1] > 1:
        top = torch.topk(r64, 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 2 * limit
    else:
        clear = torch.ones(r64.shape[0], dtype=torch.bool)
    assert torch.equal(idx[clear], r64.argmax(dim=1)[clear]), "%s: arg-max differs from fp64's at a clear margin" % what
    return int(clear.sum())
