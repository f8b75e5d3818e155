"""The v4 graph-linear tile's dynamic LDS layout (csrc/sd_gl4_lds.h): one description that the
kernels and their launchers both read.  A stand-alone program checks it under
AddressSanitizer + UBSan.  No GPU; the device cases that run every phase are in
tests/test_gpu_kernels.py, test_gpu_configs.py and test_gpu_final_pair.py."""
import os
import re
import subprocess

import pytest

from conftest import REPO
from skeletondiffusion_amd import isa_check


def test_gl4_lds_layout_under_asan(tmp_path):
    """tests/host/gl4_lds_check.cpp: for every (J, CT, MODE, PREC) the v4 file can instantiate x ntypes
    1..J the bytes equal the launchers' earlier expressions (and gl4_pair's literal), the regions live
    at the same time are disjoint and inside the total (Y and Z aliased in MODE 3 only), and every
    offset a lane forms from the slab strides lies inside its region; MODE 2, J = 16 is 39,168 bytes
    and MODE 3, J = 16 is 52,992."""
    cxx = os.path.join(isa_check.LLVM_BIN, "clang++")
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "gl4_lds_check")
    src = os.path.join(REPO, "tests", "host", "gl4_lds_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"gl4 lds layout ok \((\d+) layouts, (\d+) offsets\)", r.stdout)
    assert m, r.stdout[-500:]
    layouts, offsets = map(int, m.groups())
    # per J and precision: MODE 0 with 1..3 column tiles, MODE 1, 2, 3 with theirs; each x ntypes 1..J
    assert layouts == sum(J * 3 * 6 for J in (16, 17, 21))
    assert offsets > 100000
    # ... which covers what the file instantiates: node counts from with_J only, 1..3 column tiles
    hip = open(os.path.join(REPO, "skeletondiffusion_amd", "csrc", "sd_graph_linear_v4.hip")).read()
    assert re.findall(r"std::integral_constant<int, (\d+)>\{\}", hip) == ["16", "17", "21"]
    tiles = re.findall(r"gl4_launch(?:_t)?<(\w+), (\d), (\d), (\d)[,>]", hip)
    assert len(tiles) > 20 and all(j in ("J", "16", "17", "21") and ct in "123" for j, _, _, ct in tiles), tiles
