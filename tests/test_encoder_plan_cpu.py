"""The encoder's host plan (csrc/ahv_enc_plan.h) on the CPU: a small program includes the header, prints plan_encoder(B) and both
workspace sizes for B = 1 .. 130, and every row is compared with a restatement of the conditions as they stood in
forward_2d3d / run_block_pair / launch_linear before the plan existed -- the restatement is the specification, in the manner of
tests/fused_cases.py for plan_score_launch.  The header is plain C++17: the host compiler builds it, no ROCm needed.
"""
import os
import shutil
import subprocess

import pytest

from .conftest import REPO

CSRC = os.path.join(REPO, "3dahv_amd", "csrc")
BS = range(1, 131)

PROGRAM = r"""
#include <cstdio>
#include "ahv_enc_plan.h"
int main()
{
    for (int B = 1; B <= 130; ++B) {
        const ahv::EncPlan p = ahv::plan_encoder(B);
        printf("%d %d %d %d %d %d %d %d %d %zu %zu\n", B, p.M, (int)p.attn_per_pair, (int)p.tile64, (int)p.ff_tiled, p.ff_out_ks,
               (int)p.ff_out_in_part, (int)p.conv_tiled, p.conv_ks, ahv::plan_transformer_workspace_floats(B),
               ahv::plan_forward_2d3d_workspace_floats(B));
    }
    printf("0 %zu %zu\n", ahv::plan_transformer_workspace_floats(0), ahv::plan_forward_2d3d_workspace_floats(-3));
    return 0;
}
"""


def restated(B):
    """(M, attention per pair, 64-tiles, FF tiled, FF-out K split, FF-out slabs in `part`, conv tiled, conv K split)."""
    M = 64 * B
    attn_per_pair = 8 * B >= 192
    tile64 = M >= 2048 and M % 64 == 0 and all(n % 64 == 0 for n in (768, 256, 512))
    ff_tiled = M >= 1024 and M % 128 == 0
    ff_out_ks = (8 if M <= 1024 else 4) if ff_tiled else (8 if M <= 128 else 4)
    conv_tiled = M >= 1024 and M % 64 == 0
    conv_ks = (1 if M >= 4096 else 4096 // M) if conv_tiled else 9
    # the 8 slabs went behind the gated activations in `part`, the 4 into the qkv + kv scratch
    return (M, int(attn_per_pair), int(tile64), int(ff_tiled), ff_out_ks, int(ff_out_ks == 8), int(conv_tiled), conv_ks)


def transformer_floats(B):
    return 2 * 64 * max(B, 0) * (768 + 512 + 256 + 512 + 4096 + 256) + 64


def forward_floats(B):
    return 2 * 64 * max(B, 0) * (768 + 2304 + 6 * 256 + 128 + 128) + transformer_floats(B) + 64


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, clang++ or $CXX)"
    d = tmp_path_factory.mktemp("enc_plan")
    src, exe = str(d / "plan.cpp"), str(d / "plan")
    with open(src, "w") as f:
        f.write(PROGRAM)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe], capture_output=True, text=True,
                           timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def test_plan_matches_the_restated_conditions(rows):
    plans = [r for r in rows if r[0] > 0]
    assert [r[0] for r in plans] == list(BS)
    for r in plans:
        assert r[1:9] == restated(r[0]), "B = %d" % r[0]


def test_the_restatement_has_every_edge_in_range():
    """Both sides of every decision occur in B = 1 .. 130, at the batch sizes tests/test_gpu_encoder_bytes.py records."""
    col = lambda i: {B: restated(B)[i] for B in BS}
    assert (col(1)[23], col(1)[24]) == (0, 1)
    assert (col(2)[31], col(2)[32], col(2)[63], col(2)[64]) == (0, 1, 1, 1)
    assert (col(3)[15], col(3)[16], col(3)[17], col(3)[18]) == (0, 1, 0, 1)
    assert [col(4)[B] for B in (2, 3, 15, 16, 17, 18)] == [8, 4, 4, 8, 4, 4]
    assert [col(7)[B] for B in (15, 16, 17, 21, 22, 32, 33, 63, 64, 130)] == [9, 4, 3, 3, 2, 2, 1, 1, 1, 1]


def test_workspace_sizes_are_the_closed_forms(rows):
    for r in rows:
        B = r[0]
        assert r[-2:] == (transformer_floats(B), forward_floats(B)), "B = %d" % B
    assert rows[-1] == (0, 64, 128)   # B <= 0: no rows, the two tails
