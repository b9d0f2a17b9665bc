#!/usr/bin/env python3
"""Record tests/golden/encoder_kernels_recorded.npz and encoder_kernels_recorded_b17.npz: what the encoder kernels
(csrc/ahv_encoder.hip and the ahv_enc_*.h it includes) write for the inputs of tests/encoder_bytes_inputs.py -- a SHA-256 per
output sample of forward_2d3d and of ahv_transformer_blocks_f32 at every batch size next to a host decision, and the volumes
of B = 3 and 17 in full (those of B = 17 in the second file).  Needs the MI355X and a built library.

Run it on the commit whose bytes are to be pinned, BEFORE a change that must not move them; tests/test_gpu_encoder_bytes.py then
holds every later build to the recording.  Run on an unchanged build it reproduces the committed files bit for bit.

    python tools/gen_golden_encoder.py [--out tests/golden] [--lib path/to/libahv_hip.so]
"""
import argparse
import importlib
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def save(path, arrays):
    """np.savez_compressed with a fixed member date: the same arrays give the same file, whenever it is written."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"), help="directory")
    ap.add_argument("--lib", help="the build to record from (the parent's); default: the library in the tree")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gen_golden_encoder.py records on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    from tests import encoder_bytes_inputs as eb
    if a.lib:
        ahv._lib.LIB_PATH = os.path.abspath(a.lib)
    ahv._lib.load()
    fa = eb.make_aligner(ahv)
    rec = {}
    for B in eb.FORWARD_BS:
        for name, data in eb.recompute_forward(fa, B):
            assert name not in rec
            rec[name] = data.copy()
    for B in eb.BLOCKS_BS:
        for name, data in eb.recompute_blocks(fa, B):
            assert name not in rec
            rec[name] = data.copy()
    torch.cuda.synchronize()
    os.makedirs(a.out, exist_ok=True)
    for name, keep in eb.FILES.items():
        path = os.path.join(a.out, name + ".npz")
        packed = eb.pack(rec, keep)
        save(path, packed)
        size = os.path.getsize(path)
        print("%d entries, %d bytes recorded, %d bytes -> %s" % (len(packed["names"]), packed["data"].size, size, path))
        assert size <= 1 << 20, "above the size limit for a committed file"


if __name__ == "__main__":
    main()
