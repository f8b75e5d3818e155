"""Host walk of the diversity ranking's kernels: tests/host/rank_emulation.cpp includes
skeletondiffusion_amd/csrc/sd_rank_addr.h, the index arithmetic, orderings and reduction steps the kernels
call, and runs as a program of its own under AddressSanitizer + UBSan.  No GPU, nothing preloaded; the device
tests are in tests/test_gpu_rank.py."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO


def test_kernels_share_the_header_with_the_host_program():
    """The kernels call the header's functions (no second copy of the index arithmetic in the .hip file)."""
    hip = open(os.path.join(REPO, "skeletondiffusion_amd", "csrc", "sd_rank.hip")).read()
    hdr = open(os.path.join(REPO, "skeletondiffusion_amd", "csrc", "sd_rank_addr.h")).read()
    assert '#include "sd_rank_addr.h"' in hip
    for fn in ("pair_tiles", "point_offset", "dist_offset", "owns", "meet", "block_best", "min_nan", "anchored", "a_slot",
               "b_slot", "load_row", "load_kq", "out_row", "out_col", "chunk_quads"):
        assert re.search(rf"\b{fn}\b", hdr) and re.search(rf"\b{fn}(<\w+>)?\(", hip), fn
    from skeletondiffusion_amd import build
    assert "sd_rank.hip" in build.SOURCES and "sd_rank_addr.h" in build.HEADERS


def test_index_walk_and_greedy_under_asan(tmp_path):
    """Phase 1: every load, LDS slot and store of every workgroup for samples + 1 in {2, 63, 64, 65, 256} and
    features in {1, 9, 32, 33}: in bounds, every matrix entry written once, bitwise the chunked chain of
    sd_cdist, symmetric, zero diagonal.  Phase 2: the workgroup's shuffle tree in lockstep on matrices with
    ties, duplicates and NaN against a restatement with double keys."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rank_emulation")
    src = os.path.join(REPO, "tests", "host", "rank_emulation.cpp")
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"rank emulation ok \((\d+) matrix cases, (\d+) accesses, (\d+) selection cases\)", r.stdout)
    assert m and int(m.group(1)) == 20 and int(m.group(2)) > 0 and int(m.group(3)) >= 7 * 4 * 2, r.stdout
