"""Inputs, references and the yardstick for the encoder feed-forward under autograd
(``aligner._FF``: cat[x, m] (512) -> Linear(512 -> 2 x 2048) -> val * gelu(gate) -> Linear(2048 -> 256), fp32,
M = 64 B token rows).  No GPU is touched here: this is what a HIP forward + backward of that module is to be held against.

* Inputs are seeded: the stock ``_FF(512, 256)`` with ``nn.Linear``'s default initialisation, ``randn`` tokens and
  ``randn`` output gradients, B samples of 64 tokens.
* References: that module under fp64 CPU autograd (``ref64``) and under fp32 CPU autograd (``ref32``).
* Yardstick, as in tests/backward_cases.py: per tensor (y, dx, dw1, db1, dw2, db2) the error is the largest absolute
  difference over the largest absolute entry of ``ref64``; ``e_ref`` is that error for ``ref32`` and the bar is
  ``min(GRAD_RTOL, PARITY_FACTOR * e_ref)``.
"""
import copy
import functools
import importlib
import zlib

import torch

from .backward_cases import PARITY_FACTOR
from .backward_reference import GRAD_RTOL, relerr

TENSORS = ("y", "dx", "dw1", "db1", "dw2", "db2")
KINDS = ("plain", "wide_gate", "zero_bias", "sparse_grad")
FF_IN, FF_INNER, FF_OUT = 512, 2048, 256
TOKENS = 64
WIDE_GATE_SCALE = 8.0

# B: M = 64 (less than a 128-row tile), 192 (one and a half), 576, 1024 / 1088 (either side of a 1024-term chain over M),
# 2112 (an odd count past the training batch).  A kernel whose launch rule turns elsewhere below 33 adds those B.
SIZES = (1, 3, 9, 16, 17, 33)

# e_ref as measured on the CPU over SIZES x plain and B = 3 x KINDS (lowest, highest).  It moves with the thread count of
# the CPU's blocked sums; tests/test_ff_train_cases_cpu.py accepts a factor of two either side.
E_REF_MEASURED = {
    "y": (3.4e-7, 6.8e-7),
    "dx": (4.4e-7, 5.9e-7),
    "dw1": (5.5e-7, 8.3e-7),
    "db1": (3.1e-7, 5.5e-7),
    "dw2": (5.1e-7, 7.4e-7),
    "db2": (8.4e-8, 1.7e-7),
}


def stock_ff():
    aligner = importlib.import_module("3dahv_amd.aligner")
    return aligner._FF(FF_IN, FF_OUT)


class Case:
    """One (kind, B): fp32 CPU inputs ``x (B, 64, 512)``, ``gy (B, 64, 256)``, ``w1, b1, w2, b2``; ``ref64`` / ``ref32``
    dicts over TENSORS (token tensors flattened to M rows); ``e_ref`` and ``bars`` per tensor."""

    def __init__(self, kind, B):
        assert kind in KINDS
        self.kind, self.B, self.M = kind, B, TOKENS * B
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(zlib.crc32(("ff_train %s %d" % (kind, B)).encode()))
            ff = stock_ff()
            x = torch.randn(B, TOKENS, FF_IN)
            gy = torch.randn(B, TOKENS, FF_OUT)
        p1, p2 = ff.net[0].proj, ff.net[2]
        with torch.no_grad():
            if kind == "wide_gate":      # gates span +-20: both GELU tails, the dip near -0.75, the underflow of gelu'
                p1.weight[FF_INNER:] *= WIDE_GATE_SCALE
            elif kind == "zero_bias":
                p1.bias.zero_()
                p2.bias.zero_()
            elif kind == "sparse_grad":  # no gradient on every second token
                gy[:, 1::2] = 0.0
        self.x, self.gy = x, gy
        self.w1, self.b1 = p1.weight.detach().clone(), p1.bias.detach().clone()
        self.w2, self.b2 = p2.weight.detach().clone(), p2.bias.detach().clone()
        self.ref64 = self._reference(ff, torch.float64)
        self.ref32 = self._reference(ff, torch.float32)
        self.e_ref = {k: relerr(self.ref32[k], self.ref64[k]) for k in TENSORS}
        self.bars = {k: min(GRAD_RTOL, PARITY_FACTOR * self.e_ref[k]) for k in TENSORS}

    def _reference(self, ff, dtype):
        m = copy.deepcopy(ff).to(dtype)
        x = self.x.to(dtype).requires_grad_(True)
        y = m(x)
        y.backward(self.gy.to(dtype))
        p1, p2 = m.net[0].proj, m.net[2]
        out = {"y": y.detach(), "dx": x.grad, "dw1": p1.weight.grad, "db1": p1.bias.grad, "dw2": p2.weight.grad,
               "db2": p2.bias.grad}
        return {k: (v.reshape(-1, v.shape[-1]) if v.dim() == 3 else v).detach() for k, v in out.items()}

    def gates(self):
        """The gate pre-activations in fp64, (M, 2048)."""
        return (self.x.double().reshape(self.M, FF_IN) @ self.w1.double().t() + self.b1.double())[:, FF_INNER:]

    def errors(self, got):
        """{tensor: error of ``got[tensor]`` on the yardstick} for a dict over TENSORS on any device."""
        return {k: relerr(got[k].detach().cpu().reshape(self.ref64[k].shape), self.ref64[k]) for k in TENSORS}


@functools.lru_cache(maxsize=None)
def case(kind, B):
    """Built once per session and shared: treat it as read-only."""
    return Case(kind, B)


def all_cases():
    """(kind, B): every size with plain data, and every kind at B = 3."""
    return [("plain", B) for B in SIZES] + [(k, 3) for k in KINDS if k != "plain"]
