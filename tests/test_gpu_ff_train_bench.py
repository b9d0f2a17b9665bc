"""tools/bench_ff_train.py on the GPU, at its smallest: one sample, one round of two iterations per window."""
import importlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_measure_gives_every_row_and_restores_the_blas_choice():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        tool = importlib.import_module("bench_ff_train")
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))
    before = torch.backends.cuda.preferred_blas_library()
    seen = []
    rows = tool.measure(rounds=1, iters=2, batches=(1,), emit=seen.append)
    assert torch.backends.cuda.preferred_blas_library() == before
    assert rows == seen and len(rows) == 6
    assert [(r["row"], r["what"].split()[-1], r["blas"]) for r in rows] == [
        ("F", "fwd", "hipBLASLt"), ("F", "fwd_bwd", "hipBLASLt"), ("F", "fwd", "rocBLAS"), ("F", "fwd_bwd", "rocBLAS"),
        ("E", "feed-forwards)", "hipBLASLt"), ("E", "feed-forwards)", "rocBLAS")]
    for r in rows:
        assert r["B"] == 1 and 0 < r["min_us"] <= r["us"] <= r["max_us"] and r["rounds"] == 1
        assert r["device"] == torch.cuda.get_device_name(0)
        if r["row"] == "F":
            assert r["M"] == 64 and r["iters"] == 2 and 0 < r["frac_fp32_matrix_peak"] < 1   # no faster than the matrix peak
        else:
            assert r["iters"] == 1 and r["ff_share"] > 0
    only_e = tool.measure(only="E", rounds=1, iters=2, batches=(1,))
    assert [r["row"] for r in only_e] == ["E", "E"] and all("ff_share" not in r for r in only_e)
