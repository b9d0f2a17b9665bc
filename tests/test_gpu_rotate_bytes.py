"""The rotate_volume family's outputs, bit for bit, against the bytes recorded from the library before its five kernels moved to
csrc/ahv_rotate.hip and were given one trilinear rule (tests/golden/rotate_kernels_recorded.npz, written by
tools/gen_golden_rotate.py from the inputs of tests/rotate_bytes_inputs.py).  The fp64 comparisons of test_gpu_parity.py,
test_gpu_rotate_volume_grad.py and test_gpu_rotation_grad.py allow a regrouped sum or a differently contracted coordinate; this
does not: the clamp, the floor, the in-range test per corner, the order of the corner sums and of the nine-sum reduction, the
NaN a non-finite volume or rotation reports and the exact gather all show here.  The volume adjoint sums with float atomics
and is pinned only on inputs whose partial sums are exact (rotate_bytes_inputs has the argument); its tolerance test is
test_gpu_boundary.py's.
"""
import numpy as np
import pytest
import torch

from . import rotate_bytes_inputs as rb
from .conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(ahv):
    ahv._lib.load()
    return ahv.ops


@pytest.fixture(scope="module")
def recorded():
    return rb.unpack(load_golden("rotate_kernels_recorded"))


def test_every_recorded_array_belongs_to_a_family(recorded):
    assert recorded and all(k.startswith(rb.FAMILIES) for k in recorded)


@pytest.mark.parametrize("family", rb.FAMILIES)
def test_bytes_are_the_recorded_ones(ops, dev, recorded, family):
    """Every case of the family (rotate_bytes_inputs lists them): whole outputs, or their sha256 with the first and the last
    hypothesis; exactly the recorded set, nothing skipped."""
    seen = set()
    for name, words in rb.recompute(ops, dev, family):
        assert name not in seen and np.array_equal(np.asarray(words), recorded[name]), name
        seen.add(name)
    assert seen == {k for k in recorded if k.startswith(family)}
