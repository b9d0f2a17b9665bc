"""The tracking kernels' outputs, bit for bit, against the bytes recorded from the library before its tracking code moved to
csrc/ahv_track.hip and the two smoothers were given one pairwise walk (tests/golden/track_kernels_recorded.npz, written by
tools/gen_golden_track.py from the inputs of tests/track_bytes_inputs.py).  The fp64 comparisons of test_gpu_smooth.py and
test_gpu_marginal.py allow a regrouped sum; this does not: the 16 x 16 split of the marginal sums, the order of their merges,
every first-arg-max tie, the ring's slot arithmetic and the predict step's instruction sequence all show here.
"""
import numpy as np
import pytest
import torch

from . import track_bytes_inputs as tb
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
    return tb.unpack(load_golden("track_kernels_recorded"))


def _compare(recorded, pairs):
    seen = 0
    for name, words in pairs:
        assert torch.equal(words.reshape(-1), torch.from_numpy(np.ascontiguousarray(recorded[name]))), name
        seen += 1
    return seen


@pytest.mark.parametrize("M", tb.MS)
def test_smoother_bytes_are_the_recorded_ones(ops, dev, recorded, M):
    """Per frame delta, back, alpha, emit; at the end hist_P (M <= 257), the backtrace at F = 1 and H, the marginals at
    F = 1, 2 and H -- for the chain with velocities and jump = 8 and for the one without and jump = +inf."""
    seen = _compare(recorded, tb.recompute(ops, dev, M))
    assert seen == sum(1 for k in recorded if k.startswith("M%d_" % M)) + (len(tb.CHAINS) - 1) * tb.FRAMES


def test_predict_step_bytes_are_the_recorded_ones(ops, dev, recorded):
    """diffuse_rotations and predict_rotations over every combination of the grid at M = 2, 255 and 257 (the whole output, or
    the edge slots of track_bytes_inputs.predict_cases at the large M), and track_advance's u."""
    seen = _compare(recorded, tb.recompute_predict(ops, dev))
    assert seen == sum(1 for k in recorded if k.startswith(("diffuse_", "predict_", "advance")))
