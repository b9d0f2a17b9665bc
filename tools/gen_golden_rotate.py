#!/usr/bin/env python3
"""Record tests/golden/rotate_kernels_recorded.npz: the bytes the rotate_volume family (the forward's two kernels, the volume
adjoint, the rotation gradient's two kernels, score_rotation_grad) writes for the inputs of tests/rotate_bytes_inputs.py, as raw
32-bit words or their sha256.  Needs the MI355X and a built library.

Run it on the commit whose bytes are to be pinned, BEFORE a change that must not move them; tests/test_gpu_rotate_bytes.py then
holds every later build to the recording.  ``--lib`` records from another build of the same ABI (the parent's, built in a copy
of the tree) without touching the in-tree one.

    python tools/gen_golden_rotate.py [--lib PATH/libahv_hip.so] [--out tests/golden/rotate_kernels_recorded.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def save(path, rec):
    """One archive member for all the words, as tools/gen_golden_track.py writes it: ``names``, ``sizes`` and the arrays' int32
    words back to back in that order (tests/rotate_bytes_inputs.py ``unpack``)."""
    names = sorted(rec)
    np.savez_compressed(path, names=np.array(names), sizes=np.array([rec[n].size for n in names], np.int64),
                        words=np.concatenate([rec[n].reshape(-1) for n in names]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rotate_kernels_recorded.npz"))
    ap.add_argument("--lib", default=None, help="record from this libahv_hip.so instead of the in-tree build")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gen_golden_rotate.py records on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    if a.lib:
        ahv._lib.LIB_PATH = os.path.abspath(a.lib)
    from tests import rotate_bytes_inputs as rb
    ahv._lib.load()
    dev = torch.device("cuda:0")
    rec = {}
    for family in rb.FAMILIES:
        for name, words in rb.recompute(ahv.ops, dev, family):
            assert name not in rec and name.startswith(family), name
            rec[name] = np.array(words)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    save(a.out, rec)
    print("%s: %d arrays, %d words, %d bytes -> %s" % (ahv._lib.LIB_PATH, len(rec), sum(v.size for v in rec.values()),
                                                       os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
