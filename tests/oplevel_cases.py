"""Inputs, references and the acceptance rule for the op-level kernels (csrc/ahv_ops.hip: the three forward_3d2d kernels
and score_features; csrc/ahv_rotate.hip: rotate_volume and its volume adjoint), shared by tests/test_oplevel_cases_cpu.py
(the conditions the cases must meet, no GPU) and tests/test_gpu_oplevel_edges.py (the kernels at every dispatch path and
grid edge).

Inputs: every item of a batch is independent random data, so an item read from or written to the wrong place is an O(1)
error, and the heads are random too (`head`), so a fragment-layout error cannot hide behind the one golden head.

References: oracle/torch_ref.py's forward_3d2d / rotate_volume and the literal score expression on the CPU, in fp64 on
the same fp32 values cast up (`ref64`) and in fp32 (`ref32`).

The yardstick comes from the reference alone: for a case, e_ref = max|ref32 - ref64| and e_got = max|got - ref64| over the
elements that are finite in ref32, and the case passes when e_got <= MARGIN * e_ref.  Kernel and ref32 are both fp32
evaluations of one expression in different summation orders.  MARGIN = 4: the kernels contract 384 products as 96 sequential
MFMA steps of 4 where the reference runs a blocked, vectorised GEMM, and random-walk growth puts the longer chain at about
twice a blocked sum; the other factor of two covers the spread between the maxima of two independent error samples of one
size.  The bound therefore follows the head and the data of each case; nothing in it is calibrated against the kernels.
"""
import functools
import importlib
import os

import numpy as np
import torch

from oracle import torch_ref

MARGIN = 4.0
OLD_TENSOR_RTOL = 1e-5          # tests/test_gpu_parity.py: max|diff| / max|ref| over a whole tensor
CU_MI355X = 256                 # what the CPU test sizes the cases with; the GPU test asks the device
KINDS = ("plain", "no_bias", "dead_relu", "clamp", "golden")
EPS = 1e-12                     # F.normalize's clamp_min
QNAN, PINF, NINF = 0x7FC00000, 0x7F800000, 0xFF800000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOL = (16, 8, 8, 8)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- sizes ---------------------------------------------------------------------------------------------------------------
def forward_path(M):
    """Which kernel launch_forward_3d2d takes for M items."""
    return "small" if M <= 64 else ("dual" if M >= 4096 else "mid")


def sizes(cu):
    """The item counts of the forward_3d2d cases for a device of `cu` compute units, each checked to land where it is meant
    to (grids: mid min((M+3)/4, cu) workgroups of 4 waves, dual min((M+7)/8, cu) workgroups of 8 waves)."""
    s = {"small": (1, 2, 63, 64),
         "mid_first": 65,                 # 17 workgroups, three idle waves in the last
         "mid_second_pass": 4 * cu + 3,   # a second pass taken by three waves only
         "mid_last": 4095,
         "dual_first": 4096,
         "dual_lone_third_pass": 16 * cu + 1,    # a third pass by one wave, which prefetches its own quarter 0
         "dual_ragged_third_pass": 17 * cu + 45}  # a third pass that ends inside wave 1's row of workgroups
    assert all(forward_path(m) == "small" for m in s["small"])
    for k in ("mid_first", "mid_second_pass", "mid_last"):
        assert forward_path(s[k]) == "mid", (k, s[k], cu)
    for k in ("dual_first", "dual_lone_third_pass", "dual_ragged_third_pass"):
        assert forward_path(s[k]) == "dual", (k, s[k], cu)
    assert (s["mid_first"] + 3) // 4 <= cu and s["mid_first"] % 4 == 1
    assert s["mid_second_pass"] - 4 * min((s["mid_second_pass"] + 3) // 4, cu) == 3
    assert s["mid_last"] > 4 * cu
    for k, tail in (("dual_lone_third_pass", 1), ("dual_ragged_third_pass", cu + 45)):
        grid = min((s[k] + 7) // 8, cu)
        assert grid == cu and s[k] - 16 * grid == tail and tail < 8 * grid   # two full passes, then `tail` items
    return s


def rotate_sizes(cu):
    """N for the rotate_volume cases: the fast kernel's grid is capped at 3 cu workgroups of 4 hypotheses, the generic
    forward's and the adjoint's at 16 cu workgroups of 256 voxels (plane = 4*6*5 = 120 voxels per hypothesis)."""
    fast = 12 * cu + 5
    plane = 4 * 6 * 5
    generic = (16 * cu * 256) // plane + 1 + 7
    assert (generic - 7) * plane > 16 * cu * 256 >= (generic - 8) * plane
    return {"fast": fast, "generic": generic}


def score_sizes(cu):
    """(B, N) for score_features: one wave per (b, n), 4 per workgroup, the grid capped at 8 cu workgroups."""
    big = (2, 16 * cu + 3)
    assert big[0] * big[1] - 32 * cu == 6      # six waves into a second pass
    return [(1, 1), (3, 5), (5, 3), big]


# ---- forward_3d2d inputs -------------------------------------------------------------------------------------------------
def head(seed, kind="plain"):
    """(W1 (32,384), W2 (32,32), b2 (32,)): W1 ~ N(0, 1/384), W2 ~ N(0, 1/32), b2 ~ N(0, 1); see KINDS."""
    assert kind in KINDS, kind
    if kind == "golden":
        g = np.load(os.path.join(GOLDEN, "score_n128.npz"), allow_pickle=False)
        return tuple(torch.from_numpy(np.ascontiguousarray(g[k])).reshape(s) for k, s in
                     (("W1", (32, 384)), ("W2", (32, 32)), ("b2", (32,))))
    g = _gen(seed)
    W1 = torch.randn(32, 384, generator=g) * (1.0 / 384) ** 0.5
    W2 = torch.randn(32, 32, generator=g) * (1.0 / 32) ** 0.5
    b2 = torch.randn(32, generator=g)
    if kind in ("no_bias", "clamp"):
        b2 = torch.zeros(32)
    if kind == "dead_relu":
        W1 = -W1.abs()
    return W1, W2, b2


CLAMP_SPREAD = (0.5, 0.8, 1.0, 1.25, 2.0)


def clamp_scale(x, hd):
    """The factor that puts the MEDIAN fp64 column norm of forward_3d2d's pre-normalised output at EPS.  With b2 = 0 the
    head is positively homogeneous, so the norms at scale s are s times those at scale 1; those are read off the reference
    itself on a probe small enough (1e-14) that every column is clamped: the output's norm is then |v| / EPS."""
    assert not hd[2].any()
    probe = 1e-14
    out = ref64("forward_3d2d", x[:32] * probe, *hd)
    norms = out.norm(dim=1) * EPS / probe
    assert float(out.norm(dim=1).max()) < 0.5, "probe not clamped"
    return float(EPS / norms.median())


def items(M, seed, kind="plain", hd=None):
    """(M,16,8,8,8) independent randn items.  dead_relu: |randn| (with W1 <= 0 every pre-activation is <= 0).  clamp
    (needs the head): scaled to ~1e-13 so that the median column norm is EPS, item i by CLAMP_SPREAD[i % 5] more."""
    x = torch.randn(M, *VOL, generator=_gen(seed))
    if kind == "dead_relu":
        x = x.abs()
    if kind == "clamp":
        f = torch.tensor([CLAMP_SPREAD[i % len(CLAMP_SPREAD)] for i in range(M)])
        x = x * (clamp_scale(x, hd) * f).float().reshape(M, 1, 1, 1, 1)
    return x


def plant(x, where):
    """A copy of `x` with the bit patterns of `where` = [(item, (c, d, h, w), bits), ...] written over single voxels."""
    y = x.clone()
    v = y.view(torch.int32)
    for m, (c, d, h, w), bits in where:
        v[m, c, d, h, w] = bits - (1 << 32) if bits >= (1 << 31) else bits
    return y


def nonfinite_plan(M):
    """One quiet NaN, one +inf and one -inf voxel in three different items (first pass, the middle, the LAST item), at
    voxels whose three image positions (h,w), (d,w), (d,h) are distinct."""
    assert M >= 3
    return [(min(5, M - 3), (3, 1, 6, 2), QNAN), (M // 2 + 1 if M > 4 else 1, (15, 7, 0, 4), PINF), (M - 1, (0, 2, 5, 7), NINF)]


# ---- references ----------------------------------------------------------------------------------------------------------
def _score_literal(f_src, f_tgt):
    return (f_src * f_tgt[:, None]).sum(2).mean(-1)


def _rotate(vol, R):
    """vol (N,...) per sample, or (1,...) shared by all of R (expanded AFTER the cast, never materialised)."""
    if vol.shape[0] == 1 and R.shape[0] > 1:
        vol = vol.expand(R.shape[0], -1, -1, -1, -1)
    return torch_ref.rotate_volume(vol, R)


def _rotate_adjoint(vol_like, R, grad_out):
    """d <grad_out, rotate_volume(vol, R)> / d vol by torch autograd (linear in vol: its values do not matter).  vol_like
    (1,...) with more rotations: the shared volume, all hypotheses summed into one."""
    vol = torch.zeros_like(vol_like, requires_grad=True)
    with torch.enable_grad():
        _rotate(vol, R).backward(grad_out)
    return vol.grad


U32 = 2.0 ** -24        # unit roundoff of fp32


CHAIN_Z = 8.0


def adjoint_chain_allowance(like, R, grad_out):
    """What ONE fp32 accumulator per element costs the shared-volume adjoint: per element and in fp64, the standard deviation
    of the chain's running error averaged over the orders the adds can land in, and the mean chain length.

    rotate_volume_backward_kernel adds every term t = w * g (a trilinear corner weight times an output gradient) into its
    element of grad_vol with a float atomic.  With one volume shared by N hypotheses an element is a chain of up to 8 N adds
    (41 000 on average at N = 8 746 on (3,4,6,5)), where the CPU reference first sums each hypothesis' handful of terms and
    then reduces the N volumes blockwise.  MARGIN's premise -- a longer chain is about twice a blocked sum -- does not cover
    a chain that long.  The running error of s_k = fl(s_{k-1} + t_k) is sum_k d_k s_k with |d_k| <= U32, so with independent
    uniform d_k its standard deviation is at most U32 sqrt(sum_k s_k^2 / 3).  The order of the atomics is the hardware's; over
    random orders of the n terms of an element (sum S, sum of squares T2) the partial sum after k terms has mean S k/n and
    variance T2 (k/n)(1 - k/n), so E sum_k s_k^2 = n (S^2 / 3 + T2 / 6) and

        sd = U32 sqrt(n (S^2 / 3 + T2 / 6) / 3).

    The bar is CHAIN_Z = 8 of these: 4 for the normal tail over the few hundred elements of a volume, times 2 because
    sum_k s_k^2 of the ONE order that happened is itself spread about its mean -- the integral of a squared Brownian bridge
    exceeds 4 times its mean with probability ~exp(-pi^2 / 3) = 4 %, 9 times with ~6e-4 -- which with the normal tail of
    what is left comes to ~1e-5 per element.

    The corner enumeration restates F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False) as
    oracle/torch_ref.py calls them; its sum is checked against the fp64 autograd reference right here."""
    N, (C, D, H, W) = R.shape[0], like.shape[1:]
    assert like.shape[0] == 1 and tuple(grad_out.shape) == (N, C, D, H, W)
    plane = D * H * W
    Rd, g = R.double(), grad_out.double().reshape(N, C, plane)
    axis = lambda n: (2.0 * torch.arange(n, dtype=torch.float64) + 1.0) / n - 1.0
    pz, py, px = torch.meshgrid(axis(D), axis(H), axis(W), indexing="ij")
    p = torch.stack([px, py, pz], -1).reshape(plane, 3)
    q = torch.einsum("nij,vj->nvi", Rd, p)                                      # (N, plane, xyz)
    coord = [((q[..., a] + 1.0) * n - 1.0) / 2.0 for a, n in ((0, W), (1, H), (2, D))]
    lo = [c.floor() for c in coord]
    n_adds = torch.zeros(plane, dtype=torch.float64)
    S, T2 = torch.zeros(C, plane, dtype=torch.float64), torch.zeros(C, plane, dtype=torch.float64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = lo[0] + dx, lo[1] + dy, lo[2] + dz
                wx, wy, wz = (1 - (coord[a] - i).abs() for a, i in ((0, ix), (1, iy), (2, iz)))
                w = wx * wy * wz
                ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H) & (iz >= 0) & (iz < D) & (w != 0)   # what the kernel adds
                dst = ((iz * H + iy) * W + ix).long()[ok]
                n_adds.index_add_(0, dst, torch.ones_like(dst, dtype=torch.float64))
                for c in range(C):
                    t = (w * g[:, c])[ok]
                    S[c].index_add_(0, dst, t)
                    T2[c].index_add_(0, dst, t * t)
    want = ref64("rotate_volume_adjoint", like, R, grad_out).reshape(C, plane)
    assert (S - want).abs().max() <= 1e-11 * want.abs().max(), "the corner enumeration is not the reference's"
    sd = U32 * (n_adds[None] * (S * S / 3.0 + T2 / 6.0) / 3.0).sqrt()
    return sd.reshape(like.shape), int(n_adds.mean())


def _score_hypotheses(vol_src, vol_tgt, R, W1, W2, b2):
    """torch_ref.score_hypotheses' scores (B,N), in chunks of 256 hypotheses.  It takes R (N,3,3) shared by the batch; for
    R (B,N,3,3) per sample it is called sample by sample (tests/fused_cases.py)."""
    if R.dim() == 3:
        return torch_ref.score_hypotheses(vol_src, vol_tgt, R, W1, W2, b2, chunk=256)[0]
    return torch.cat([torch_ref.score_hypotheses(vol_src[b:b + 1], vol_tgt[b:b + 1], R[b], W1, W2, b2, chunk=256)[0]
                      for b in range(R.shape[0])])


_OPS = {"forward_3d2d": torch_ref.forward_3d2d, "rotate_volume": _rotate, "score_features": _score_literal,
        "rotate_volume_adjoint": _rotate_adjoint, "score_hypotheses": _score_hypotheses}


def _ref(dtype, op, *args):
    with torch.no_grad():
        return _OPS[op](*(a.detach().cpu().to(dtype) for a in args))


def ref64(op, *args):
    """`op` on the CPU in fp64, the fp32 inputs cast up."""
    return _ref(torch.float64, op, *args)


def ref32(op, *args):
    """`op` on the CPU in fp32: the reference as it runs."""
    return _ref(torch.float32, op, *args)


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def errors(got, r32, r64, where=None):
    """(e_got, e_ref) over the elements finite in ref32 (and selected by the boolean tensor `where`, if given)."""
    got = got.detach().cpu()
    assert got.shape == r32.shape == r64.shape and got.dtype == r32.dtype == torch.float32 and r64.dtype == torch.float64
    fin = torch.isfinite(r32)
    if where is not None:
        fin = fin & where
    assert fin.any(), "nothing to compare"
    assert torch.isfinite(got[fin]).all(), "non-finite output where the reference is finite"
    e_ref = float((r32.double() - r64)[fin].abs().max())
    e_got = float((got.double() - r64)[fin].abs().max())
    return e_got, e_ref


def accept(got, r32, r64, what, where=None, old_bar=False):
    """The rule: e_got <= MARGIN * e_ref.  Prints the figures first (a run with -s records them) and returns
    e_got / e_ref.  old_bar: also require that MARGIN * e_ref is no looser than OLD_TENSOR_RTOL * max|ref|."""
    e_got, e_ref = errors(got, r32, r64, where)
    assert e_ref > 0.0, what + ": fp32 reference equals fp64, no yardstick"
    print("%-58s e_got %.3e  e_ref %.3e  e_got/e_ref %.2f" % (what, e_got, e_ref, e_got / e_ref))
    if old_bar:
        assert_not_weaker(r32, r64, what)
    assert e_got <= MARGIN * e_ref, "%s: e_got %.3e above %g x e_ref %.3e (ratio %.2f)" % (
        what, e_got, MARGIN, e_ref, e_got / e_ref)
    return e_got / e_ref


def assert_not_weaker(r32, r64, what):
    fin = torch.isfinite(r32)
    e_ref = float((r32.double() - r64)[fin].abs().max())
    old = OLD_TENSOR_RTOL * float(r64[fin].abs().max())
    assert MARGIN * e_ref <= old, "%s: %g x e_ref = %.3e is looser than the old bar %.3e" % (what, MARGIN, MARGIN * e_ref, old)


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """Inputs of one case with its two references (all on the CPU)."""

    def __init__(self, name, args, r32, r64, kind=None):
        self.name, self.args, self.r32, self.r64, self.kind = name, args, r32, r64, kind


def _seed(kind, M):
    return 1000 * KINDS.index(kind) + M


@functools.lru_cache(maxsize=3)
def forward_case(M, kind="plain"):
    """forward_3d2d on M items with the head of `kind`; seeds follow from (kind, M) alone."""
    hd = head(7 + KINDS.index(kind), kind)
    x = items(M, _seed(kind, M), kind, hd)
    args = (x,) + tuple(hd)
    return Case("forward_3d2d M=%d %s" % (M, kind), args, ref32("forward_3d2d", *args), ref64("forward_3d2d", *args), kind)


def clamp_masks(case):
    """(clamped, unclamped) boolean masks over the output elements of a clamp case, by the fp64 reference's column norm."""
    clamped = (case.r64.norm(dim=1, keepdim=True) < 1.0 - 1e-9).expand_as(case.r64)
    return clamped, ~clamped


def dead_relu_column(hd):
    """b2 / |b2| in fp64: what every output column of a dead_relu case is."""
    b = hd[2].double()
    return b / b.norm()


def nonfinite_case(M):
    """(clean items, planted items, plan, head, ref32 and ref64 of the three flagged items alone -- items are independent)."""
    base = forward_case(M, "plain")
    x, hd = base.args[0], base.args[1:]
    plan = nonfinite_plan(M)
    bad = plant(x, plan)
    idx = [m for m, _, _ in plan]
    assert len(set(idx)) == 3
    return x, bad, plan, hd, ref32("forward_3d2d", bad[idx], *hd), ref64("forward_3d2d", bad[idx], *hd)


INF_ROWS = (3, 20)


def inf_column_case(M):
    """A +inf voxel whose column holds +-inf AND NaN before it is normalised: column k of W1 (the z slab's channel of the
    voxel) is made negative except in rows INF_ROWS, so at position (h, w) exactly two hidden units are +inf (the rest are
    relu(-inf) = 0) and v_k = W2[k, r0] inf + W2[k, r1] inf + finite is +-inf where the two weights agree in sign and NaN where
    they do not.  The column's norm is NaN, F.normalize's clamp_min keeps it NaN, and the reference's whole column is NaN;
    a clamp that DROPS the NaN (fmaxf) would leave +-inf in it.  Returns (clean items, planted items, flagged item, head,
    ref32 and ref64 of the flagged item)."""
    base = forward_case(M, "plain")
    x = base.args[0]
    W1, W2, b2 = (t.clone() for t in base.args[1:])
    m, (c, d, h, w) = M // 2, (9, 4, 3, 5)
    k = 256 + 8 * c + d                 # torch_ref.forward_3d2d: slabs = [along_x | along_y | along_z], along_z channel 8 c + d
    W1[:, k] = -W1[:, k].abs()
    W1[list(INF_ROWS), k] *= -1
    agree = torch.sign(W2[:, INF_ROWS[0]]) == torch.sign(W2[:, INF_ROWS[1]])
    assert agree.any() and not agree.all()
    bad = plant(x, [(m, (c, d, h, w), PINF)])
    hd = (W1, W2, b2)
    return x, bad, m, hd, ref32("forward_3d2d", bad[m:m + 1], *hd), ref64("forward_3d2d", bad[m:m + 1], *hd)


def features(B, N, seed):
    """f_src (B,N,32,64) and f_tgt (B,32,64) with unit-norm columns (what forward_3d2d hands to the score)."""
    g = _gen(seed)
    f_src = torch.nn.functional.normalize(torch.randn(B, N, 32, 64, generator=g), dim=2)
    f_tgt = torch.nn.functional.normalize(torch.randn(B, 32, 64, generator=g), dim=1)
    return f_src, f_tgt


@functools.lru_cache(maxsize=2)
def score_case(B, N):
    args = features(B, N, 5000 + 100 * B + N)
    return Case("score_features B=%d N=%d" % (B, N), args, ref32("score_features", *args), ref64("score_features", *args))


def _haar(n, seed):
    return torch.from_numpy(importlib.import_module("3dahv_amd.rotations").haar_rotations_np(n, seed))


@functools.lru_cache(maxsize=2)
def rotate_case(which, cu):
    """which = 'fast': one (16,8,8,8) volume shared by 12 cu + 5 Haar rotations (args: vol (1,...), R).
    'generic': (3,4,6,5) per sample at the first N past one grid, plus 7, Haar rotations.
    'adjoint_per': the same shape and N, random R (every fourth scaled by 1.7: corners leave the volume), args (vol_like,
    R, grad_out), the reference is torch autograd.  'adjoint_shared': the same with ONE volume for all hypotheses."""
    n = rotate_sizes(cu)
    g = _gen({"fast": 6001, "generic": 6002, "adjoint_per": 6003, "adjoint_shared": 6004}[which])
    if which == "fast":
        args = (torch.randn(1, *VOL, generator=g), _haar(n["fast"], 6011))
        op = "rotate_volume"
    elif which == "generic":
        args = (torch.randn(n["generic"], 3, 4, 6, 5, generator=g), _haar(n["generic"], 6012))
        op = "rotate_volume"
    else:
        N = n["generic"]
        R = _haar(N, 6013) + 0.1 * torch.randn(N, 3, 3, generator=g)
        R[::4] *= 1.7
        shape = (1 if which == "adjoint_shared" else N, 3, 4, 6, 5)
        args = (torch.zeros(shape), R, torch.randn(N, 3, 4, 6, 5, generator=g))
        op = "rotate_volume_adjoint"
    return Case("rotate_volume %s N=%d" % (which, args[1].shape[0]), args, ref32(op, *args), ref64(op, *args))
