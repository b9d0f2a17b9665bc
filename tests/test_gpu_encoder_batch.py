"""The encoder's HIP kernels (csrc/ahv_encoder.hip, ahv_enc_*.h) on batches of DISTINCT samples at every edge of the host dispatch
(forward_2d3d / run_block_pair), against the fp64 copy of the same module under the per-sample rule of
tests/encoder_reference.py: each sample at most 3 x as far from fp64 as the worst sample of the stock fp32 operators, in
max and in rms, no additive floor.  Beside it: zero padding carrying the whole signal, sample isolation and batch order
bit for bit, independence of what the workspace held (with guard bands around every buffer the C ABI writes), large gates
through both GEGLU epilogues, and graph replay at B = 16.

Largest observed ratios (worst HIP sample / worst stock fp32 sample, over all cases of the item; MI355X, larger of two
runs -- the stock side moves by a few per cent between runs; the bar is 3):

    item                                            emax_hip / emax_stock   erms_hip / erms_stock
    1  forward_2d3d, distinct samples, 13 B x 2            1.9                     1.6
    1  att(x, c) alone, 6 B x 2                            1.1                     0.9
    2  border tokens only                                  1.3                     0.9
    2  one token per sample                                1.0                     1.0
    6  large gates, B = 3 / 16                             0.9                     0.9

(largest absolute figures, item 1: emax 1.4e-5 for the HIP kernels, 2.0e-5 for the stock fp32 operators.)
Items 3, 4, 5 and 7 are bit-for-bit and hold as written: no kernel of the forward sums in a position-dependent order.

Checked against deliberately wrong builds (not kept): one tap of the tiled 3 x 3 convolution reading the sample two
further on passes every test of tests/test_gpu_encoder.py at B = 16, 32, 64 (its batches tile two stored samples) and fails
items 1, 2 and 3 here at every B >= 16; the zero row left uncleared together with one GELU coefficient off in its third
digit (9e-6 in GELU) passes all of tests/test_gpu_encoder.py and fails items 1 (att), 2, 3 and 5 here.
"""
import copy
import ctypes

import pytest
import torch

from . import encoder_reference as ref

pytestmark = pytest.mark.gpu

# what each B selects, read from plan_encoder (csrc/ahv_enc_plan.h; M = 64 B rows per stream)
EDGES = {
    3: "skinny conv, gridDim.z 3",
    8: "skinny conv, gridDim.z 8",
    15: "last skinny conv",
    16: "conv K-split 4, FF-out tiled split-K 8",
    17: "conv K-split 3, odd row count, skinny FF",
    18: "conv K-split 3, tiled FF split-K 4, attention per key tile",
    21: "last conv K-split 3",
    22: "first conv K-split 2",
    23: "last B on attention_heads_kernel",
    24: "first B on attention_sample_head_kernel",
    32: "last conv K-split 2, 64-tiles for the 256-wide linears",
    33: "conv K-split 1, 64-tiles beside skinny FF",
    64: "the M >= 4096 branch",
}
BATCHES = [pytest.param(B, id="B%d-%s" % (B, what.replace(" ", "_").replace(",", ""))) for B, what in EDGES.items()]
WEIGHTS = ["seed0", "procedural"]


@pytest.fixture(scope="module")
def aligners(ahv):
    """{name: (module, its fp64 copy)}: the 768 -> 256, 4-head, depth-4 aligner with torch's default initialisation
    (seed 0, as tests/test_gpu_encoder.py) and a second one carrying the key-seeded procedural weights (every norm gain
    and bias non-trivial)."""
    from .procfill import procedural_state_dict
    make = lambda: ahv.aligner.Feature_Aligner(in_channel=768, mid_channel=256, out_channel=32, n_heads=4, depth=4).eval()
    torch.manual_seed(0)
    seed0 = make().cuda()
    proc = make()
    proc.load_state_dict(procedural_state_dict(proc.state_dict()), strict=True)
    proc = proc.cuda()
    return {"seed0": (seed0, ref.double_copy(seed0)), "procedural": (proc, ref.double_copy(proc))}


def layer4_pair(B, seed):
    """2 B independent (768, 8, 8) samples, sample i of the 2 B scaled by SCALES[i % 5] (source and target of a pair
    differ in scale too)."""
    return ref.scaled_samples(B, (768, 8, 8), seed).cuda(), ref.scaled_samples(B, (768, 8, 8), seed + 1000, first=B).cuda()


def check_forward(fa, fa64, a, b, what):
    got, stock, want = ref.hip32(fa, a, b), ref.stock32(fa, a, b), ref.truth(fa, a, b, fa64)
    for name, x, s, t in zip(("vol_src", "vol_tgt"), got, stock, want):
        assert x.shape == (a.shape[0], 16, 8, 8, 8)
        ref.accept(x, s, t, "%s %s" % (what, name))


# ---- 1. distinct samples at every dispatch edge ------------------------------------------------------------------
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("B", BATCHES)
def test_forward_2d3d_distinct_samples(aligners, B, weights):
    fa, fa64 = aligners[weights]
    a, b = layer4_pair(B, 100 + B)
    check_forward(fa, fa64, a, b, "forward_2d3d %s B=%d" % (weights, B))


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("B", [2, 15, 18, 22, 23, 64])   # the sizes test_transformer_blocks_match_torch_ops leaves out
def test_transformer_distinct_samples(aligners, B, weights):
    fa, fa64 = aligners[weights]
    x = ref.scaled_samples(B, (256, 8, 8), 200 + B).cuda()
    c = ref.scaled_samples(B, (256, 8, 8), 1200 + B, first=B).cuda()
    got, stock, want = ref.hip32(fa.att, x, c), ref.stock32(fa.att, x, c), ref.truth(fa.att, x, c, fa64.att)
    for name, g, s, t in zip(("x", "context"), got, stock, want):
        ref.accept(g, s, t, "att %s B=%d %s" % (weights, B, name))


# ---- 2. zero padding carries the signal ----------------------------------------------------------------------------
def border_only(B, seed):
    keep = torch.zeros(8, 8)
    keep[0], keep[7], keep[:, 0], keep[:, 7] = 1, 1, 1, 1
    assert int(keep.sum()) == 28
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 768, 8, 8, generator=g) * keep).cuda(), (torch.randn(B, 768, 8, 8, generator=g) * keep).cuda()


def one_token(B, seed):
    """One non-zero token per sample: a corner (all four in turn) for even i, (3, 4) for odd i."""
    corners = ((0, 0), (0, 7), (7, 0), (7, 7))
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        t = torch.zeros(B, 768, 8, 8)
        for i in range(B):
            y, x = corners[(i // 2) % 4] if i % 2 == 0 else (3, 4)
            t[i, :, y, x] = torch.randn(768, generator=g)
        out.append(t.cuda())
    return out


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("pattern", ["border", "one_token"])
@pytest.mark.parametrize("B", [3, 16, 17, 33])   # skinny conv; tiled conv with K split 4, 3 and 1
def test_forward_2d3d_signal_at_the_zero_padding(aligners, B, pattern, weights):
    fa, fa64 = aligners[weights]
    a, b = (border_only if pattern == "border" else one_token)(B, 300 + B)
    check_forward(fa, fa64, a, b, "%s %s B=%d" % (pattern, weights, B))


# ---- 3. sample isolation, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_forward_2d3d_sample_isolation(aligners, B):
    fa, _ = aligners["procedural"]
    a, b = layer4_pair(B, 400 + B)
    base = ref.hip32(fa, a, b)
    g = torch.Generator().manual_seed(500 + B)
    others = lambda j: [i for i in range(B) if i != j]
    for j in sorted({0, B // 2, B - 1}):
        a2, b2 = a.clone(), b.clone()
        a2[j], b2[j] = torch.randn(768, 8, 8, generator=g).cuda(), torch.randn(768, 8, 8, generator=g).cuda()
        for what, (aa, bb) in (("both inputs", (a2, b2)), ("the target input", (a, b2))):
            got = ref.hip32(fa, aa, bb)
            for name, x, y in zip(("vol_src", "vol_tgt"), got, base):
                keep = others(j)
                same = (x[keep] == y[keep]).flatten(1).all(1)
                assert bool(same.all()), "%s of sample %d replaced: %s of samples %s changed" % (
                    what, j, name, [keep[i] for i in (~same).nonzero().flatten().tolist()])
                # cross attention: a new target changes the source volume too
                assert not torch.equal(x[j], y[j]), "%s of sample %d replaced: its %s did not change" % (what, j, name)


# ---- 4. batch order, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_forward_2d3d_batch_order(aligners, B):
    """Every sample moves to another tile, tile half and workgroup; the kernels have no atomics and a fixed split-K order, so a
    row's arithmetic does not depend on where it sits."""
    fa, _ = aligners["procedural"]
    a, b = layer4_pair(B, 600 + B)
    base = ref.hip32(fa, a, b)
    got = ref.hip32(fa, a.flip(0), b.flip(0))
    for name, x, y in zip(("vol_src", "vol_tgt"), got, base):
        same = (x.flip(0) == y).flatten(1).all(1)
        assert bool(same.all()), "%s of samples %s depends on the batch order" % (name, (~same).nonzero().flatten().tolist())


# ---- 5. workspace content and bounds ---------------------------------------------------------------------------------
GUARD = 4096
PATTERN = 0xA5


class Guarded:
    """`nbytes` bytes as a 256-byte-aligned interior slice of a larger buffer, a 4 KiB band of PATTERN before and after."""

    def __init__(self, nbytes, device):
        assert nbytes % 4 == 0
        self.raw = torch.full((nbytes + 2 * GUARD + 256,), PATTERN, dtype=torch.uint8, device=device)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.nbytes = nbytes
        self.f32 = self.raw[self.off:self.off + nbytes].view(torch.float32)
        assert self.f32.data_ptr() % 256 == 0 and self.f32.numel() * 4 == nbytes

    def ptr(self):
        return self.f32.data_ptr()

    def guards_intact(self):
        before, after = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        assert before.numel() >= GUARD and after.numel() >= GUARD
        return bool((before == PATTERN).all()) and bool((after == PATTERN).all())


def abi_forward_2d3d(ahv, fa, a, b, fill):
    """ahv_forward_2d3d_f32 as hip_forward_2d3d calls it, on guarded buffers, the workspace pre-filled with `fill`."""
    lib, B, dev = ahv._lib.load(), a.shape[0], a.device
    packed = fa._pack_aligner(dev)
    ws = Guarded(lib.ahv_forward_2d3d_workspace_bytes(B), dev)
    vols = [Guarded(B * 16 * 512 * 4, dev) for _ in range(2)]
    ws.f32.fill_(fill)
    with torch.cuda.device(dev):
        ahv._lib.check(lib.ahv_forward_2d3d_f32(ctypes.byref(packed.table), a.data_ptr(), b.data_ptr(), B, ws.ptr(), ws.nbytes,
                                                vols[0].ptr(), vols[1].ptr(), torch.cuda.current_stream(dev).cuda_stream),
                       "ahv_forward_2d3d_f32")
    torch.cuda.synchronize(dev)
    for name, buf in zip(("workspace", "vol_src", "vol_tgt"), [ws] + vols):
        assert buf.guards_intact(), "forward_2d3d wrote outside its %s (B = %d)" % (name, B)
    return [v.f32.clone().reshape(B, 16, 8, 8, 8) for v in vols]


def abi_transformer_blocks(ahv, att, xs, cs, fill):
    """ahv_transformer_blocks_f32 as BidirectionTransformer._hip_blocks calls it: in-place token buffers, all guarded."""
    lib, B, dev = ahv._lib.load(), xs.shape[0], xs.device
    table = att._pack(dev).table
    ws = Guarded(lib.ahv_transformer_workspace_bytes(B), dev)
    toks = [Guarded(B * 64 * 256 * 4, dev) for _ in range(2)]
    toks[0].f32.copy_(xs.flatten())
    toks[1].f32.copy_(cs.flatten())
    ws.f32.fill_(fill)
    with torch.cuda.device(dev):
        ahv._lib.check(lib.ahv_transformer_blocks_f32(table, len(att.transformer_blocks), toks[0].ptr(), toks[1].ptr(), B,
                                                      ws.ptr(), ws.nbytes, torch.cuda.current_stream(dev).cuda_stream),
                       "ahv_transformer_blocks_f32")
    torch.cuda.synchronize(dev)
    for name, buf in zip(("workspace", "x_src", "x_tgt"), [ws] + toks):
        assert buf.guards_intact(), "transformer_blocks wrote outside its %s (B = %d)" % (name, B)
    return [t.f32.clone().reshape(B, 64, 256) for t in toks]


FILLS = [0.0, float("nan"), 1e30]


@pytest.mark.parametrize("B", [2, 16, 33])   # skinny conv (no zero row read); tiled conv with K split 4 and 1
def test_forward_2d3d_workspace_content_and_bounds(ahv, aligners, B):
    fa, _ = aligners["seed0"]
    a, b = layer4_pair(B, 700 + B)
    outs = [abi_forward_2d3d(ahv, fa, a, b, fill) for fill in FILLS]
    for fill, out in zip(FILLS, outs):
        for name, x, y in zip(("vol_src", "vol_tgt"), out, outs[0]):
            assert torch.isfinite(x).all(), "%s not finite after a workspace of %r" % (name, fill)
            assert torch.equal(x, y), "%s depends on what the workspace held (%r against 0)" % (name, fill)
    for x, y in zip(outs[0], ref.hip32(fa, a, b)):   # the helper runs what the product runs
        assert torch.equal(x, y)


@pytest.mark.parametrize("B", [2, 16, 33])
def test_transformer_blocks_workspace_content_and_bounds(ahv, aligners, B):
    att = aligners["seed0"][0].att
    g = torch.Generator().manual_seed(800 + B)
    xs, cs = torch.randn(B, 64, 256, generator=g).cuda(), torch.randn(B, 64, 256, generator=g).cuda()
    outs = [abi_transformer_blocks(ahv, att, xs, cs, fill) for fill in FILLS]
    for fill, out in zip(FILLS, outs):
        for name, x, y in zip(("x", "context"), out, outs[0]):
            assert torch.isfinite(x).all(), "%s not finite after a workspace of %r" % (name, fill)
            assert torch.equal(x, y), "%s depends on what the workspace held (%r against 0)" % (name, fill)
    with torch.no_grad():
        for x, y in zip(outs[0], att._hip_blocks(xs, cs)):
            assert torch.equal(x, y)


# ---- 6. large gates through both GEGLU epilogues -----------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 16])   # linear_staged_kernel<2, 512, true>; linear_tile_kernel<true, 4>
def test_geglu_epilogues_with_large_gates(aligners, B):
    """A depth-1 slice with the gate half of every ff.net.0.proj.weight x 30: gates of +-17 rms reach far into both tails of
    gelu_pk (the fitted range ends at |g| = 6), where a wrong coefficient or a missing monotone fall shows."""
    att1 = copy.deepcopy(aligners["seed0"][0].att)
    att1.transformer_blocks = torch.nn.ModuleList([att1.transformer_blocks[1]])
    with torch.no_grad():
        for blk in (getattr(att1.transformer_blocks[0], n) for n in ("attn_self_1", "attn_self_2", "attn_cross_1", "attn_cross_2")):
            w = blk.ff.net[0].proj.weight
            w[w.shape[0] // 2:].mul_(30.0)   # _GatedProj: chunk(2) -> (value, gate)
    att1.invalidate_packed()
    blk64 = ref.double_copy(att1.transformer_blocks[0])
    g = torch.Generator().manual_seed(900 + B)
    xs, cs = torch.randn(B, 64, 256, generator=g).cuda(), torch.randn(B, 64, 256, generator=g).cuda()
    with torch.no_grad():
        gate = att1.transformer_blocks[0].attn_self_1.ff.net[0].proj(torch.cat([xs, xs], 2))[..., 2048:]
        assert gate.abs().max() > 30 and (gate.abs() < 1).any()   # both the tails and the fitted range are visited
        stock = att1.transformer_blocks[0](xs, cs)
        got = att1._hip_blocks(xs, cs)
        want = blk64(xs.double(), cs.double())
    for name, x, s, t in zip(("x", "context"), got, stock, want):
        ref.accept(x, s, t, "geglu B=%d %s" % (B, name))


# ---- 7. graph replay off the B = 1 path ---------------------------------------------------------------------------------
def test_graphed_forward_2d3d_at_batch_16(aligners):
    fa, _ = aligners["procedural"]
    run = fa.graphed_forward_2d3d(batch=16)
    for k in range(3):
        a, b = layer4_pair(16, 950 + k)
        out = run(a, b)
        want = ref.hip32(fa, a, b)
        for name, x, y in zip(("vol_src", "vol_tgt"), out, want):
            assert torch.equal(x, y), "replay %d: %s differs from the eager HIP call" % (k, name)
