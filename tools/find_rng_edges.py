#!/usr/bin/env python3
"""Walks the Haar stream of one seed with the numpy mirror (tests/rng_reference.py) and prints the first offset of each of the
three reachable corners of box_muller4 (3dahv_amd/csrc/ahv_so3.h), which a random case meets about once in 2^24 blocks:

  radius_zero   word0 >> 8 == 0xFFFFFF   u0 = 1, log = 0: the first two quaternion components are exactly 0
  radius_max    word0 >> 8 == 0          u0 = 2^-24: the largest radius, sqrt(48 ln 2) = 5.768
  angle_zero    word1 >> 8 == 0          u1 = 0: the angle is exactly 0, the second component exactly 0

The offsets go into tests/rng_cases.py (EDGE_SEED, EDGE_OFFSETS); the tests recompute only those blocks.  No GPU.

    python tools/find_rng_edges.py [--seed S] [--chunk-log2 22] [--max-log2 30]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import rng_reference as rr  # noqa: E402

KINDS = {"radius_zero": (0, 0xFFFFFF), "radius_max": (0, 0), "angle_zero": (1, 0)}      # name -> (word, value of word >> 8)


def search(seed, chunk_log2=22, max_log2=30):
    found, chunk = {}, 1 << chunk_log2
    k0, k1 = seed & rr.M32, (seed >> 32) & rr.M32
    for start in range(0, 1 << max_log2, chunk):
        ctr = np.arange(start, start + chunk, dtype=np.uint64)
        words = rr.philox4x32_10(ctr & np.uint64(rr.M32), ctr >> np.uint64(32), rr.HAAR_TAG, 0, k0, k1)
        for name, (w, value) in KINDS.items():
            if name not in found:
                hit = np.flatnonzero((words[w] >> np.uint32(8)) == np.uint32(value))
                if hit.size:
                    found[name] = start + int(hit[0])
        if len(found) == len(KINDS):
            break
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x3DA4F)
    ap.add_argument("--chunk-log2", type=int, default=22)
    ap.add_argument("--max-log2", type=int, default=30)
    a = ap.parse_args()
    t = time.time()
    found = search(a.seed, a.chunk_log2, a.max_log2)
    print("EDGE_SEED = 0x%X" % a.seed)
    print("EDGE_OFFSETS = {%s}" % ", ".join('"%s": %d' % (k, found[k]) for k in KINDS if k in found))
    missing = [k for k in KINDS if k not in found]
    print("# %d blocks walked in %.0f s%s" % (max(found.values(), default=0) + 1, time.time() - t,
                                               "; not found below 2^%d: %s" % (a.max_log2, ", ".join(missing)) if missing else ""))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
