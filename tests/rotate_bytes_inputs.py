"""Inputs, and the one call sequence, of the recorded bytes of the rotate_volume family (tests/golden/rotate_kernels_recorded.npz):
tools/gen_golden_rotate.py records what ``recompute`` yields and tests/test_gpu_rotate_bytes.py compares against it, so the
fixture holds outputs only.  The inputs are seeded numpy (``RandomState``), ``rotations.haar_rotations_np`` and the goldens
score_n128, edge_rotations and nonfinite; tests/rotate_grad_reference.py and the two gradient tests supply their own cases.

Families (the prefix of a recorded name), each the smallest shapes at which a path of its kernels can still go wrong:
  "rot_"   rotate_volume, the (16,8,8,8) kernel on a shared volume: N = 1, N = 5 (a ragged last workgroup), N = 3 077 (past
           the 3 x 256 x 4 hypotheses a launch holds at once: the grid-stride loop and the prefetch clamp), the edge_rotations
           set, and a NaN and an inf voxel at N = 5 (every hypothesis through the exact gather)
  "gen_"   rotate_volume, the generic kernel: (3,4,6,5) per sample at N = 7, (1,8,8,8) shared at N = 64, (16,8,8,8) per
           sample at N = 9 (stride != 0: not the fast kernel), (3,4,6,5) at N = 9 000 (past the 16 x 256 x 256 threads)
  "rvg_"   rotate_volume_rotation_grad: every case of tests/test_gpu_rotate_volume_grad.py, (3,4,6,5) at N = 2 100 (past the
           8 x 256 workgroups), a NaN and an inf entry of R for either kernel
  "srg_"   score_rotation_grad: B x N = 1 x 1, 1 x 1 024, 3 x 37 with per-sample R (make_case of
           tests/test_gpu_rotation_grad.py), the last also with a NaN voxel in one sample and with an inf entry of R
  "adj_"   the volume adjoint.  It sums with float atomics, so it is pinned only where the order of the adds cannot matter:
           the identity and the six axis permutations on (16,8,8,8) and (3,4,2,8) -- power-of-two sizes, every coordinate and
           weight a short dyadic fraction -- with an integer-valued grad_out, so that every partial sum is exact.  Per sample
           at N = 7, shared at N = 2.
What is stored per case: the whole output as int32 words where it is at most 48 KB, else a sha256 of its bytes plus the first
and the last hypothesis in full, or (``DIGEST_ONLY``) the sha256 alone -- the fixture stays under 256 KB.
"""
import hashlib
import importlib
import itertools

import numpy as np

from . import rotate_grad_reference as rg
from .conftest import load_golden

rot = importlib.import_module("3dahv_amd.rotations")

FAMILIES = ("rot_", "gen_", "rvg_", "srg_", "adj_")
WHOLE_MAX_BYTES = 48 * 1024
# cases above WHOLE_MAX_BYTES whose hypotheses are 32 KB each and add nothing at their ends: the digest alone
DIGEST_ONLY = {"rot_N5", "rot_edge_rotations", "rot_nan_voxel", "rot_inf_voxel", "gen_N9_16x8x8x8_per"}
# (N, C, D, H, W, shared volume?, seed) through rotate_grad_reference.random_case
GENERIC = [(7, 3, 4, 6, 5, False, 420), (64, 1, 8, 8, 8, True, 421), (9, 16, 8, 8, 8, False, 422), (9000, 3, 4, 6, 5, False, 423)]
RVG_LARGE = (2100, 3, 4, 6, 5, False, 424)
RVG_BAD_R = (37, 33)                                   # N of the rows of test_gpu_rotate_volume_grad.CASES: one per kernel
SRG = [(1, 1, False, 300), (1, 1024, False, 350), (3, 37, True, 370)]     # (B, N, per-sample R?, seed)
ADJ_SHAPES = [(16, 8, 8, 8), (3, 4, 2, 8)]
ADJ_SEED = 430


def unpack(recorded):
    """The fixture as {name: flat int32 words}."""
    ends = np.cumsum(recorded["sizes"])
    words = recorded["words"]
    return {str(n): words[e - k:e] for n, k, e in zip(recorded["names"], recorded["sizes"], ends)}


def _entries(name, out):
    """(name, int32 words) of what is stored for the output ``out`` (hypotheses along dim 0) of case ``name``."""
    import torch
    w = out.detach().contiguous().cpu().view(torch.int32).numpy()
    if w.nbytes <= WHOLE_MAX_BYTES:
        yield name, w.reshape(-1)
        return
    yield name + "_sha256", np.frombuffer(hashlib.sha256(w.tobytes()).digest(), np.int32)
    if name not in DIGEST_ONLY:
        yield name + "_first", w[0].reshape(-1)
        yield name + "_last", w[-1].reshape(-1)


def _shared(vol, N):
    return vol[None].expand(N, -1, -1, -1, -1)


def _on(dev, vol, R, g=None):
    """The case on the device; a shared volume stays a stride-0 expand of one."""
    vol = _shared(vol[0].to(dev), vol.shape[0]) if vol.stride(0) == 0 and vol.shape[0] > 1 else vol.to(dev)
    return (vol, R.to(dev)) if g is None else (vol, R.to(dev), g.to(dev))


def _plant(t, index, bits):
    """A copy of ``t`` with the 32-bit pattern ``bits`` at ``index``."""
    import torch
    a = t.numpy().copy()
    a.view(np.uint32)[index] = bits
    return torch.from_numpy(a)


def axis_permutations():
    """(7,3,3): the identity, then the six permutation matrices of the axes (the identity among them)."""
    mats = [np.eye(3, dtype=np.float32)]
    for p in itertools.permutations(range(3)):
        m = np.zeros((3, 3), np.float32)
        m[np.arange(3), p] = 1.0
        mats.append(m)
    return np.stack(mats)


def recompute(ops, dev, family):
    """(name, int32 words) of everything recorded for ``family``, from the library ``ops`` drives."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    haar = rot.haar_rotations_np
    g128 = load_golden("score_n128")
    vol128 = t(g128["vol_src"])[0]

    if family == "rot_":
        edge, nf = load_golden("edge_rotations"), load_golden("nonfinite")
        sets = [("rot_N%d" % N, vol128, t(haar(N, 410 + k))) for k, N in enumerate((1, 5, 3077))]
        sets.append(("rot_edge_rotations", vol128, t(edge["R"])))
        for tag, want in (("rot_nan_voxel", "nan_centre"), ("rot_inf_voxel", "inf_face")):
            (k,) = [i for i, n in enumerate(nf["names"]) if str(n) == want]
            idx = tuple(int(i) for i in nf["index"][k] if i >= 0)[1:]          # the index into (1,16,8,8,8) without its batch
            sets.append((tag, _plant(vol128, idx, nf["bits"][k]), t(nf["R"][:5])))
        for name, vol, R in sets:
            yield from _entries(name, ops.rotate_volume(*_on(dev, _shared(vol, R.shape[0]), R)))

    elif family == "gen_":
        for N, C, D, H, W, shared, seed in GENERIC:
            vol, R, _ = rg.random_case(haar, N, C, D, H, W, shared, seed)
            name = "gen_N%d_%dx%dx%dx%d_%s" % (N, C, D, H, W, "shared" if shared else "per")
            yield from _entries(name, ops.rotate_volume(*_on(dev, vol, R)))

    elif family == "rvg_":
        from . import test_gpu_rotate_volume_grad as tv
        pkg = importlib.import_module("3dahv_amd")
        cases = [(name, case) for name, case, _ in tv.all_cases(pkg)]
        N, C, D, H, W, shared, seed = RVG_LARGE
        cases.append(("N%d_%dx%dx%dx%d_per" % (N, C, D, H, W), rg.random_case(haar, *RVG_LARGE)))
        for n in RVG_BAD_R:
            vol, R, g = tv.case_by_n(pkg, n)
            R = R.clone()
            R[3, 1, 2], R[7, 0, 0] = float("nan"), float("inf")
            cases.append(("N%d_bad_R" % n, (vol, R, g)))
        for name, case in cases:
            yield from _entries("rvg_" + name, ops.rotate_volume_rotation_grad(*_on(dev, *case)))

    elif family == "srg_":
        from . import test_gpu_rotation_grad as ts
        pkg = importlib.import_module("3dahv_amd")
        cases = [("srg_B%d_N%d" % (B, N), ts.make_case(pkg, B, N, per, seed)) for B, N, per, seed in SRG]
        vs, ft, R, W1, W2, b2, gs = cases[-1][1]
        cases.append(("srg_B3_N37_nan_voxel", (_plant(vs, (1, 7, 3, 4, 5), 0x7FC00000), ft, R, W1, W2, b2, gs)))
        cases.append(("srg_B3_N37_inf_R", (vs, ft, _plant(R, (2, 5, 1, 1), 0x7F800000), W1, W2, b2, gs)))
        for name, case in cases:
            vs, ft, R, W1, W2, b2, gs = (x.to(dev) for x in case)
            yield from _entries(name, ops.score_rotation_grad(vs, ft, R, W1, W2, b2, grad_scores=gs))

    elif family == "adj_":
        P = axis_permutations()
        rs = np.random.RandomState(ADJ_SEED)
        for shape in ADJ_SHAPES:
            for shared, pick in ((False, list(range(7))), (True, [3, 5])):
                R = t(P[pick])
                N = R.shape[0]
                g = t(rs.randint(1, 9, (N,) + shape).astype(np.float32) * rs.choice([-1.0, 1.0], (N,) + shape).astype(np.float32))
                base = torch.zeros(shape if shared else (N,) + shape, device=dev, requires_grad=True)
                ops.rotate_volume_autograd(_shared(base, N) if shared else base, R.to(dev)).backward(g.to(dev))
                grad = base.grad[None] if shared else base.grad
                yield from _entries("adj_%dx%dx%dx%d_%s" % (shape + ("shared" if shared else "per",)), grad)
    else:
        raise KeyError(family)
