"""The developer benchmark of the backward kernels compiles.  tools/kbench_bwd.cpp includes the kernel sources and names
the kernels, their launch constants and the launchers' grid / workspace helpers directly, so a change to any of them can
break it without touching the library or any other test -- it once stayed broken that way (a kernel that became a template).
Nothing runs here: both variants are cross-compiled for gfx950 with the flags of tools/build_kbench.sh."""
import os
import shutil
import subprocess

import pytest

from .conftest import REPO

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I3dahv_amd/csrc", "-Iinclude", "-Itools"]


@pytest.mark.parametrize("defines", [[], ["-DAHV_RMW_STAMPS"]], ids=["plain", "stamps"])
def test_kbench_bwd_compiles(tmp_path, defines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "kbench_bwd")
    build = subprocess.run([hipcc] + FLAGS + defines + ["tools/kbench_bwd.cpp", "-o", exe], capture_output=True, text=True,
                           timeout=900, cwd=REPO)
    assert build.returncode == 0, build.stderr[-4000:]
    assert os.path.exists(exe)
