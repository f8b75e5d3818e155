"""Host emulation of the validation-metric kernels' address arithmetic (csrc/sd_validation_addr.h, DESIGN.md
§4ad) under AddressSanitizer + UBSan, as a stand-alone program in a child process.  No GPU; the device tests
are in tests/test_gpu_validation_metrics.py."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_kernel_addresses_in_bounds_under_asan(tmp_path):
    """tests/host/validation_emulation.cpp walks every workgroup x thread x load / store of k_limb_stats,
    k_limb_reduce and k_frame_error with the kernels' own address functions: on real heap buffers at the
    fixture's and the device tests' shapes under AddressSanitizer + UBSan, arithmetically at 256 x 50 x 100 x
    16 x 3 and 256 x 50 x 120 x 21 x 3; and checks the variance combine step against two passes."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "validation_emulation")
    src = os.path.join(REPO, "tests", "host", "validation_emulation.cpp")
    # the sanitizer runtime is linked statically (g++ -static-libasan; clang's default), so the program
    # needs nothing preloaded and does not mind what its environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "validation emulation ok" in r.stdout
