"""tools/bench_ff_train.py and profiles/ff_train.jsonl without a GPU: the tool's FLOP count and feed-forward count are
the stock modules', its row arithmetic is what its docstring says, and the recorded rows are complete, consistent with that
arithmetic and the ones DESIGN.md quotes."""
import importlib
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(REPO, "profiles", "ff_train.jsonl")
STATS = ("us", "min_us", "max_us", "rounds", "iters")


@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        return importlib.import_module("bench_ff_train")
    finally:
        sys.path.remove(os.path.join(REPO, "tools"))


@pytest.fixture(scope="module")
def rows():
    with open(PROFILE) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_flop_count_and_module_count_are_the_stock_modules(tool):
    aligner = importlib.import_module("3dahv_amd.aligner")
    ff = aligner._FF(512, 256)
    macs = sum(m.weight.numel() for m in (ff.net[0].proj, ff.net[2]))      # one MAC per weight per token
    assert tool.MAC_PER_TOKEN == macs == 2_621_440
    assert tool.ff_flop(768, "fwd") == 2 * 768 * macs and tool.ff_flop(768, "fwd_bwd") == 3 * tool.ff_flop(768, "fwd")
    enc = aligner.BidirectionTransformer(256, 4, 64, depth=4)
    assert tool.N_FF == sum(isinstance(m, aligner._FF) for m in enc.modules()) == 16
    assert set(tool.BLAS.values()) == {"hipBLASLt", "rocBLAS"}


def test_row_arithmetic(tool):
    st = {"us": 100.0, "min_us": 90.0, "max_us": 130.0, "rounds": 5, "iters": 50}
    r = tool.ff_row(12, "fwd_bwd", "cublas", st)
    assert r["M"] == 768 and r["blas"] == "rocBLAS" and r["what"] == "stock _FF fwd_bwd"
    want_tf = 3 * 2 * 768 * 2_621_440 / 100e-6 / 1e12
    assert r["tflops"] == round(want_tf, 2) and r["frac_fp32_matrix_peak"] == round(want_tf / 157.3, 4)
    assert all(r[k] == st[k] for k in STATS)
    e = tool.encoder_row(12, "cublaslt", dict(st, us=8000.0), ff_fwd_bwd_us=100.0)
    assert e["ff_share"] == 0.2 and e["blas"] == "hipBLASLt" and e["us"] == 8000.0
    assert "ff_share" not in tool.encoder_row(12, "cublas", st)            # --only E: no F figure to take a share of


def test_recorded_rows_are_complete_and_follow_the_arithmetic(tool, rows):
    key = lambda r: (r["row"], r["what"].split()[-1] if r["row"] == "F" else "enc", r["B"], r["blas"])
    by = {key(r): r for r in rows}
    want = {(row, what, B, blas) for B in (12, 32) for blas in ("hipBLASLt", "rocBLAS")
            for row, what in (("F", "fwd"), ("F", "fwd_bwd"), ("E", "enc"))}
    assert set(by) == want and len(rows) == len(want)
    code = {v: k for k, v in tool.BLAS.items()}
    for (row, what, B, blas), r in by.items():
        st = {k: r[k] for k in STATS}
        assert 0 < r["min_us"] <= r["us"] <= r["max_us"] and r["rounds"] >= 5
        assert r["device"] and r["rocm"] and r["torch"]
        body = {k: v for k, v in r.items() if k not in ("device", "rocm", "torch")}
        if row == "F":
            assert body == tool.ff_row(B, what, code[blas], st)
            assert 0 < r["frac_fp32_matrix_peak"] < 1
        else:
            assert body == tool.encoder_row(B, code[blas], st, by[("F", "fwd_bwd", B, blas)]["us"])
            assert 0 < r["ff_share"] < 1
    for B in (12, 32):
        for blas in ("hipBLASLt", "rocBLAS"):   # the windows do not overlap: a backward costs more than no backward
            assert by[("F", "fwd", B, blas)]["max_us"] < by[("F", "fwd_bwd", B, blas)]["min_us"]


def test_design_quotes_the_recorded_medians(rows):
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    item = text[text.index("5. HIP forward + backward kernels for the encoder under autograd"):]
    item = item[:item.index("\n6. ")]
    assert "profiles/ff_train.jsonl" in item and "tools/bench_ff_train.py" in item
    for r in rows:
        if r["row"] == "F" and r["what"].endswith("fwd_bwd"):
            lo, hi = round(r["min_us"]), round(r["max_us"])
            assert re.search(r"%d \[%d–%d\]" % (round(r["us"]), lo, hi), item), (r["B"], r["blas"], r["us"])
        if r["row"] == "E":
            assert ("%.1f" % (r["us"] / 1e3)) in item, (r["B"], r["blas"], r["us"])
