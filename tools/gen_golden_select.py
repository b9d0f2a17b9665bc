#!/usr/bin/env python3
"""Record tests/golden/select_kernels_recorded.npz: the bytes the pose-selection kernels (keys and lists, modes, the symmetry
fold, multi-view fusion, the pose posterior, resampling, the SO(3) ascent step) write for the inputs of
tests/select_bytes_inputs.py, as raw 32-bit words or their sha256.  Needs the MI355X and a built library.

Run it on the commit whose bytes are to be pinned, BEFORE a change that must not move them -- never on the code under test;
tests/test_gpu_select_bytes.py then holds every later build to the recording.  ``--lib`` records from another build of the same
ABI (the parent's: ``make -C 3dahv_amd/csrc BUILD=/some/dir`` in a checkout of it) without touching the in-tree one.  Every
family is computed twice and must agree with itself before it is written: these kernels promise the same bytes on every run.

    python tools/gen_golden_select.py --lib PATH/libahv_hip.so [--out tests/golden/select_kernels_recorded.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MAX_BYTES = 256 * 1024


def save(path, rec):
    """One archive member for all the words, as tools/gen_golden_rotate.py writes it: ``names``, ``sizes`` and the arrays' int32
    words back to back in that order (tests/select_bytes_inputs.py ``unpack``)."""
    names = sorted(rec)
    np.savez_compressed(path, names=np.array(names), sizes=np.array([rec[n].size for n in names], np.int64),
                        words=np.concatenate([rec[n].reshape(-1) for n in names]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "select_kernels_recorded.npz"))
    ap.add_argument("--lib", default=None, help="record from this libahv_hip.so instead of the in-tree build")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gen_golden_select.py records on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    if a.lib:
        ahv._lib.LIB_PATH = os.path.abspath(a.lib)
    from tests import select_bytes_inputs as sb
    ahv._lib.load()
    dev = torch.device("cuda:0")
    rec = {}
    for family in sb.FAMILIES:
        first = {name: np.array(words) for name, words in sb.recompute(ahv.ops, dev, family)}
        again = {name: np.array(words) for name, words in sb.recompute(ahv.ops, dev, family)}
        differ = sorted(n for n in first if not np.array_equal(first[n], again.get(n)))
        if differ or set(first) != set(again):
            sys.exit("%s: two runs of %s disagree on %s" % (ahv._lib.LIB_PATH, family, differ or sorted(set(first) ^ set(again))))
        assert all(n.startswith(family) and n not in rec for n in first), family
        rec.update(first)
        print("%-7s %3d arrays, %7d words" % (family, len(first), sum(v.size for v in first.values())))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    save(a.out, rec)
    size = os.path.getsize(a.out)
    print("%s: %d arrays, %d words, %d bytes -> %s" % (ahv._lib.LIB_PATH, len(rec), sum(v.size for v in rec.values()), size, a.out))
    if size > MAX_BYTES:
        sys.exit("the fixture holds %d bytes, more than %d" % (size, MAX_BYTES))


if __name__ == "__main__":
    main()
