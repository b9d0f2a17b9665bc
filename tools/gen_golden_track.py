#!/usr/bin/env python3
"""Record tests/golden/track_kernels_recorded.npz: the bytes the tracking kernels (predict step, Viterbi and marginal smoothers)
write for the inputs of tests/track_bytes_inputs.py, as raw 32-bit words.  Needs the MI355X and a built library.

Run it on the commit whose bytes are to be pinned, BEFORE a change that must not move them; tests/test_gpu_track_bytes.py then
holds every later build to the recording.  The marginal kernels' sums depend on how the rows are split over lanes, which the
fp64 comparisons of tests/test_gpu_marginal.py cannot see; this can.

    python tools/gen_golden_track.py [--out tests/golden/track_kernels_recorded.npz]
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
    """One archive member for all the words (a member per array would cost more in headers than the small arrays hold):
    ``names``, ``sizes`` and the arrays' int32 words back to back in that order (tests/track_bytes_inputs.py ``unpack``)."""
    names = sorted(rec)
    np.savez_compressed(path, names=np.array(names), sizes=np.array([rec[n].size for n in names], np.int64),
                        words=np.concatenate([rec[n].reshape(-1) for n in names]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "track_kernels_recorded.npz"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gen_golden_track.py records on the GPU only")
    ahv = importlib.import_module("3dahv_amd")
    from tests import track_bytes_inputs as tb
    ahv._lib.load()
    dev = torch.device("cuda:0")
    rec = {}

    def record(pairs):
        for name, words in pairs:
            w = words.numpy().copy()
            if name in rec:     # emit: the same bytes from both chains
                assert np.array_equal(rec[name], w), name
            rec[name] = w

    for M in tb.MS:
        record(tb.recompute(ahv.ops, dev, M))
    record(tb.recompute_predict(ahv.ops, dev))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    save(a.out, rec)
    print("%d arrays, %d words, %d bytes -> %s" % (len(rec), sum(v.size for v in rec.values()), os.path.getsize(a.out), a.out))


if __name__ == "__main__":
    main()
