"""The encoder kernels' outputs, bit for bit, against the bytes recorded from the library before its kernels moved from
csrc/ahv_encoder.hip into ahv_enc_linear.h / ahv_enc_rows.h, linear_kernel lost its unreachable paths and the host's shape
decisions moved into ahv_enc_plan.h (tests/golden/encoder_kernels_recorded*.npz, written by tools/gen_golden_encoder.py from the
inputs of tests/encoder_bytes_inputs.py).  The fp64 comparisons of test_gpu_encoder_batch.py allow another kernel, K split or
summation order at any batch size; this does not: which kernel a launch takes, its K split, the slab order of every LayerNorm
and finish pass and every instruction sequence show here.  There is no tolerance: a difference means the arithmetic changed.
"""
import numpy as np
import pytest
import torch

from . import encoder_bytes_inputs as eb
from .conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aligner(ahv):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ahv._lib.load()
    return eb.make_aligner(ahv)


@pytest.fixture(scope="module")
def recorded():
    return eb.unpack(load_golden)


def _compare(recorded, pairs):
    seen = 0
    for name, data in pairs:
        assert name in recorded, name
        assert np.array_equal(data, recorded[name]), name
        seen += 1
    return seen


@pytest.mark.parametrize("B", eb.FORWARD_BS)
def test_forward_2d3d_bytes_are_the_recorded_ones(aligner, recorded, B):
    """Every output sample of both volumes by its SHA-256; at B = 3 and 17 the volumes themselves as well."""
    seen = _compare(recorded, eb.recompute_forward(aligner, B))
    assert seen == eb.count(recorded, "fwd", B) == 2 * B + (2 if B in eb.FULL_BS else 0)


@pytest.mark.parametrize("B", eb.BLOCKS_BS)
def test_transformer_blocks_bytes_are_the_recorded_ones(aligner, recorded, B):
    seen = _compare(recorded, eb.recompute_blocks(aligner, B))
    assert seen == eb.count(recorded, "blk", B) == 2 * B


def test_every_recorded_entry_belongs_to_a_case(recorded):
    want = sum(2 * B + (2 if B in eb.FULL_BS else 0) for B in eb.FORWARD_BS) + sum(2 * B for B in eb.BLOCKS_BS)
    assert len(recorded) == want
