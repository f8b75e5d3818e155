"""Host side of the split route's launch arguments: the work-unit decode the kernels
share with the host, the XCD remap and the packers that fill the kernels' compact argument blocks
from GLArgs, checked by a stand-alone program under AddressSanitizer + UBSan.  No GPU; the device
tests are in tests/test_gpu_launch_args.py."""
import os
import re
import subprocess

import pytest

from conftest import REPO
from skeletondiffusion_amd import isa_check

CSRC = os.path.join(REPO, "skeletondiffusion_amd", "csrc")


def _rocm_include():
    # <rocm>/lib/llvm/bin -> <rocm>/include (GLArgs names hipStream_t and _Float16: the ROCm clang builds it)
    return os.path.normpath(os.path.join(isa_check.LLVM_BIN, "..", "..", "..", "include"))


def test_decode_remap_and_packers_under_asan(tmp_path):
    """tests/host/launch_decode_check.cpp: fast_divmod against / and % for every divisor up to 4,100
    and the 32-bit edges; decode_unit + xcd_remap against the kernels' former 64-bit arithmetic for
    every workgroup of the grids J in {16, 17, 21} x row tiles in {1, 2, 8, 9, 33, 41} x column
    groups in {1, 2, 4, 8} x RT in {1, 2}; the remap a bijection with contiguous XCD shares where the
    grid is no multiple of 8; every field of every packed block against the GLArgs it came from."""
    cxx = os.path.join(isa_check.LLVM_BIN, "clang++")
    if not os.path.exists(cxx) or not os.path.exists(os.path.join(_rocm_include(), "hip", "hip_runtime.h")):
        pytest.skip("no ROCm clang++ / headers")
    exe = str(tmp_path / "launch_decode_check")
    src = os.path.join(REPO, "tests", "host", "launch_decode_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"launch decode ok \((\d+) divisions, (\d+) units, (\d+) grids\)", r.stdout)
    assert m and int(m.group(3)) >= 3 * 6 * 4 * 2, r.stdout[-500:]


def test_argument_blocks_are_whole_lines_and_division_free():
    """The blocks end on 64-byte lines under a static_assert, and the hot kernels'
    work-unit decode holds no / or % (the shared header's multiply-high form is the only one)."""
    hdr = open(os.path.join(CSRC, "sd_gl4_args.h")).read()
    for name in ("GL4GArgs", "GL4MArgs", "GL4PairArgs"):
        assert re.search(rf"static_assert\(sizeof\({name}\) % 64 == 0", hdr), name
    body = re.search(r"SD_HD void fast_divmod\(.*?\n}\n", hdr, re.S).group(0) + re.search(r"SD_HD Unit3 decode_unit\(.*?\n}\n", hdr, re.S).group(0) + \
        re.search(r"SD_HD uint32_t xcd_remap\(.*?\n}\n", hdr, re.S).group(0)
    code = re.sub(r"//.*", "", body)
    assert "/" not in code and "%" not in code, code
    src = open(os.path.join(CSRC, "sd_graph_linear_v4.hip")).read()
    # every split-route kernel decodes through the header
    for kernel, call in (("k_gl4y", "decode_unit("), ("k_gl4t", "decode_unit(xcd_remap("), ("k_gl4_pair", "fast_divmod("),
                         ("k_gl4m", "gl4_body<")):
        m = re.search(rf"void {kernel}\((.*?)\n}}\n", src, re.S)
        assert m and call in m.group(1), kernel
    for kernel, block in (("k_gl4y", "GL4GArgs"), ("k_gl4_pair", "GL4PairArgs"), ("k_gl4m", "GL4MArgs")):
        assert re.search(rf"void {kernel}\(const {block} ", src), kernel
