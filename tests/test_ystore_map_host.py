"""Host side of the split route's direct Y stores: the address map the GEMM-phase
kernels and the mixing-phase readers share (csrc/sd_ystore_map.h), checked by a stand-alone program
under AddressSanitizer + UBSan.  No GPU; the device tests are in tests/test_gpu_direct_y_store.py."""
import os
import re
import subprocess

import pytest

from conftest import REPO
from skeletondiffusion_amd import isa_check

CSRC = os.path.join(REPO, "skeletondiffusion_amd", "csrc")


def test_store_map_covers_tiles_and_matches_reader_under_asan(tmp_path):
    """tests/host/ystore_map_check.cpp: the 64 lanes x 4 stores of a tile write each of its 1,024
    floats once, each store instruction's bytes are one contiguous aligned KiB, the mixing phase's
    slab pieces are consecutive in memory, and zs_off reads back what the writer put there for N in {96, 192, 384 (paired), 768} x J in
    {16, 17, 21} x rows in {33, 257}; the same pieces on a row-major destination."""
    cxx = os.path.join(isa_check.LLVM_BIN, "clang++")
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "ystore_map_check")
    src = os.path.join(REPO, "tests", "host", "ystore_map_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"ystore map ok \((\d+) tiles, (\d+) elements, (\d+) shapes\)", r.stdout)
    assert m and int(m.group(3)) == 3 * 4 * 2 + 2, r.stdout[-500:]


def test_kernels_use_the_shared_map():
    """The writers and the readers take their addresses from the header, not from a copy."""
    src = open(os.path.join(CSRC, "sd_graph_linear_v4.hip")).read()
    assert '#include "sd_ystore_map.h"' in src
    assert "int64_t zs_off(" not in src  # defined in the header alone
    for kernel, fns in (("k_gl4y", ("ystore_zs_piece_off(", "ystore_rm_piece_off(", "ystore_col(")),
                        ("gl4t_body", ("ystore_zs_piece_off(", "ystore_col("))):
        m = re.search(rf"void {kernel}\((.*?)\n}}\n", src, re.S)
        assert m and all(f in m.group(1) for f in fns), kernel
    assert src.count("zs_strides(") >= 2 and src.count("zs_off(") >= 2 and src.count("zs_slab_piece(") >= 2
