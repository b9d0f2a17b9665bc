"""The pose-selection kernels' outputs, bit for bit, against the bytes recorded from the library before csrc/ahv_select.hip was
split into ahv_select.hip, ahv_views.hip and ahv_posterior.hip, its tile rule moved to ahv_tile.h and its wave reductions to
ahv_wave.h (tests/golden/select_kernels_recorded.npz, written by tools/gen_golden_select.py from the inputs of
tests/select_bytes_inputs.py).  The reference comparisons of test_gpu_topk.py, test_gpu_modes.py, test_gpu_sym.py,
test_gpu_views.py, test_gpu_views_compact.py, test_gpu_posterior.py and test_gpu_resample.py allow what their references allow
(a regrouped fp64 sum, a draw that sits on a boundary); this does not: the order of every sum, the shape of every wave
reduction, the tie rules, the alignment and ragged-end paths of the loaders and every launch grid show here.
"""
import numpy as np
import pytest
import torch

from . import select_bytes_inputs as sb
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
    return sb.unpack(load_golden("select_kernels_recorded"))


def test_every_recorded_array_belongs_to_a_family(recorded):
    assert recorded and all(k.startswith(sb.FAMILIES) for k in recorded)


@pytest.mark.parametrize("family", sb.FAMILIES)
def test_bytes_are_the_recorded_ones(ops, dev, recorded, family):
    """Every case of the family (select_bytes_inputs lists them): whole outputs, or their sha256 with their first and last
    words; exactly the recorded set, nothing skipped."""
    seen = set()
    for name, words in sb.recompute(ops, dev, family):
        assert name not in seen and name in recorded and np.array_equal(np.asarray(words), recorded[name]), name
        seen.add(name)
    assert seen == {k for k in recorded if k.startswith(family)}
