"""Inputs, and the one call sequence, of the recorded bytes of the encoder kernels (tests/golden/encoder_kernels_recorded*.npz):
tools/gen_golden_encoder.py records what ``recompute_forward`` / ``recompute_blocks`` yield and tests/test_gpu_encoder_bytes.py
compares against it, so the fixture holds outputs only.  Weights and inputs come from tests/procfill.py (numpy's legacy MT19937
stream seeded by SHA-256 of a key): nothing here draws from torch's generator, so a torch upgrade leaves the record valid.

Sample i of a batch (counted through source then target, as tests/test_gpu_encoder_batch.py::layer4_pair) is scaled by
``encoder_reference.SCALES[i % 5]``: a read from the wrong sample is not a small error.

Each B is the smallest batch on its side of a host decision (csrc/ahv_enc_plan.h, M = 64 B rows per stream):
  forward_2d3d   FF-out 8-way skinny (B <= 2) | 4-way; skinny | tiled FF and convolution (B >= 16, M % 128); tiled FF-out split 8
                 (B = 16) | 4; conv K split 4 / 3 / 2 / 1 (16 | 17-21 | 22-32 | >= 33; 64: M >= 4096); attention per key tile |
                 per (sample, head) (23 | 24); 64-tiles for the 256-wide linears (31 | 32; 63 | 64 for M % 64 only)
  blocks         ahv_transformer_blocks_f32 alone on token buffers (what att(x, c) runs between its stock projections): the same
                 edges of run_block_pair without the convolutions around them

Recorded: the SHA-256 of the fp32 bytes of every output sample of both streams, and both output volumes of forward_2d3d in full
at B = 3 and B = 17, so that a mismatch can be looked at.  fp32 mantissas do not deflate, and the two full batches together
(1.3 MB) are above the size limit for one committed file: the volumes of B = 17 travel in a second archive beside the first
(``FILES``).
"""
import hashlib

import numpy as np
import torch

from . import encoder_reference as ref
from .procfill import procedural_state_dict, procedural_tensor

FORWARD_BS = (1, 2, 3, 15, 16, 17, 21, 22, 23, 24, 31, 32, 33, 63, 64)
BLOCKS_BS = (2, 3, 16, 17, 24, 32)
FULL_BS = (3, 17)
STREAMS = ("src", "tgt")
# archive (under tests/golden, without .npz) -> which entries it holds
FILES = {
    "encoder_kernels_recorded": lambda name: not name.startswith("fwd_B17_") or not name.endswith("_full"),
    "encoder_kernels_recorded_b17": lambda name: name.startswith("fwd_B17_") and name.endswith("_full"),
}


def make_aligner(ahv):
    """The 768 -> 256, 4-head, depth-4 aligner with the key-seeded procedural weights, on the GPU."""
    fa = ahv.aligner.Feature_Aligner(in_channel=768, mid_channel=256, out_channel=32, n_heads=4, depth=4).eval()
    fa.load_state_dict(procedural_state_dict(fa.state_dict()), strict=True)
    return fa.cuda()


def _samples(key, B, shape, first):
    """(B, *shape) float32 of unit variance (procedural_tensor is uniform in +-1/sqrt(fan_in)), sample i scaled by
    SCALES[(first + i) % 5]."""
    x = procedural_tensor(key, (B,) + tuple(shape)) * np.float32(np.sqrt(3.0 * np.prod(shape)))
    f = np.array([ref.SCALES[(first + i) % len(ref.SCALES)] for i in range(B)], np.float32)
    return torch.from_numpy((x * f.reshape((B,) + (1,) * len(shape))).astype(np.float32))


def forward_inputs(B):
    return (_samples("encoder_bytes.layer4.src.B%d" % B, B, (768, 8, 8), 0),
            _samples("encoder_bytes.layer4.tgt.B%d" % B, B, (768, 8, 8), B))


def blocks_inputs(B):
    return (_samples("encoder_bytes.tokens.x.B%d" % B, B, (64, 256), 0),
            _samples("encoder_bytes.tokens.ctx.B%d" % B, B, (64, 256), B))


def _entries(prefix, B, outs, full):
    """(name, uint8 array) per output sample of both streams -- the 32 bytes of its SHA-256 -- and, where `full`, the whole
    stream's fp32 bytes."""
    for stream, t in zip(STREAMS, outs):
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        assert a.dtype == np.float32 and a.shape[0] == B
        for i in range(B):
            yield "%s_B%d_%s_sha_%d" % (prefix, B, stream, i), np.frombuffer(hashlib.sha256(a[i].tobytes()).digest(), np.uint8)
        if full:
            yield "%s_B%d_%s_full" % (prefix, B, stream), a.reshape(-1).view(np.uint8)


def recompute_forward(fa, B):
    """forward_2d3d through the module with every HIP switch on (encoder_reference.hip32)."""
    a, b = (t.cuda() for t in forward_inputs(B))
    outs = ref.hip32(fa, a, b)
    assert all(o.shape == (B, 16, 8, 8, 8) for o in outs)
    return _entries("fwd", B, outs, B in FULL_BS)


def recompute_blocks(fa, B):
    """ahv_transformer_blocks_f32 on token buffers (BidirectionTransformer._hip_blocks)."""
    xs, cs = (t.cuda() for t in blocks_inputs(B))
    with torch.no_grad():
        assert fa.att._hip_eligible(xs)
        outs = fa.att._hip_blocks(xs, cs)
    assert all(o.shape == (B, 64, 256) for o in outs)
    return _entries("blk", B, outs, False)


def count(recorded, prefix, B):
    return sum(1 for k in recorded if k.startswith("%s_B%d_" % (prefix, B)))


def pack(rec, keep):
    """The entries of `rec` whose name `keep` accepts, as one archive member for all the bytes: ``names``, ``sizes`` and the
    arrays back to back in that order.  The full volumes are stored byte plane by byte plane (all first bytes of the floats,
    then all second ones, ...): the exponent plane deflates well, the mantissa planes hardly."""
    names = sorted(n for n in rec if keep(n))
    parts = [rec[n].reshape(-1, 4).T.reshape(-1) if n.endswith("_full") else rec[n] for n in names]
    return dict(names=np.array(names), sizes=np.array([rec[n].size for n in names], np.int64), data=np.concatenate(parts))


def unpack(load):
    """{name: uint8 array} of every archive of ``FILES``; `load(archive name)` opens one (conftest.load_golden)."""
    out = {}
    for f in FILES:
        part = _unpack_one(load(f))
        assert not set(part) & set(out)
        out.update(part)
    return out


def _unpack_one(g):
    names, sizes, data = [str(n) for n in g["names"]], g["sizes"], g["data"]
    ends = np.cumsum(sizes)
    out = {}
    for n, e, s in zip(names, ends, sizes):
        a = data[e - s:e]
        out[n] = np.ascontiguousarray(a.reshape(4, -1).T).reshape(-1) if n.endswith("_full") else a
    return out
