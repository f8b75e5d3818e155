"""The sampling workspace's layout (csrc/sd_workspace.h): one table of buffers, and the carve, a row
chain's view and its capacities derived from it.  A stand-alone program walks it under
AddressSanitizer + UBSan; sd_workspace_bytes is pinned to recorded sizes.  No GPU; the two-chain
device test of a narrow-attention Denoiser is in tests/test_gpu_configs.py."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO
from skeletondiffusion_amd import _lib, isa_check


def test_layout_and_chain_views_under_asan(tmp_path):
    """tests/host/workspace_layout_check.cpp: for J x (D, C) x attention x rows x row_chains x cut unit
    every buffer inside the carve and 256-B aligned, the extents of any two chains disjoint in every
    buffer, every chain inside its buffer, the status word inside a 0-row carve; and the rule before
    the header (the qkv view moved by 3 hid, sized by max(3 hid, H, O)) overlapping exactly at the
    attention shapes with 3 hid < H -- heads (1, 32) and (1, 16)."""
    cxx = os.path.join(isa_check.LLVM_BIN, "clang++")
    if not os.path.exists(cxx):
        pytest.skip("no ROCm clang++")
    exe = str(tmp_path / "workspace_layout_check")
    src = os.path.join(REPO, "tests", "host", "workspace_layout_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"workspace layout ok \((\d+) shapes, (\d+) walked in memory; parent rule: (\d+) overlapping at heads "
                  r"\(1, 32\), (\d+) at \(1, 16\)\)", r.stdout)
    assert m, r.stdout[-500:]
    shapes, walked, o32, o16 = map(int, m.groups())
    assert shapes >= 4 * 3 * 5 * 11 * 8 * 2 and walked >= 100
    # (1, 32): 3 hid = 96 < H only at (D, C) = (96, 96); (1, 16): 48 < 96 and 192.  4 J, 2 units, and the
    # cells of the rows x row_chains grid that run two chains or more: 8 row counts above 32 x row_chains 2..8
    assert o32 >= 4 * 2 * 56 and o16 >= 2 * 4 * 2 * 56


# (num_nodes, latent_dim, cond_dim, attn_heads, attn_dim_head [0, 0: no attention], rows, bytes):
# sd_workspace_bytes of the library before the layout moved into sd_workspace.h
RECORDED_BYTES = [
    (16, 96, 96, 0, 0, 1, 2378240),
    (16, 96, 96, 4, 64, 400, 55083520),
    (16, 96, 96, 1, 32, 64, 5243392),
    (16, 96, 96, 1, 32, 3200, 262144512),
    (16, 96, 0, 0, 0, 33, 2968064),
    (16, 96, 0, 4, 64, 3200, 347341312),
    (16, 16, 0, 0, 0, 129, 1379840),
    (16, 16, 0, 1, 32, 32, 492032),
    (17, 96, 96, 0, 0, 1201, 118777856),
    (17, 96, 96, 1, 32, 64, 5571072),
    (17, 96, 96, 1, 32, 3200, 278528512),
    (17, 96, 0, 8, 32, 31, 3671808),
    (17, 96, 0, 1, 32, 1200, 65837568),
    (17, 16, 0, 8, 32, 50, 4899072),
    (17, 16, 0, 1, 16, 1, 282880),
    (21, 96, 96, 8, 32, 400, 72296960),
    (21, 96, 96, 1, 32, 64, 6881792),
    (21, 96, 96, 1, 32, 3200, 344064512),
    (21, 96, 96, 1, 16, 33, 6046208),
    (21, 96, 0, 8, 32, 3200, 455885312),
    (21, 96, 0, 1, 16, 129, 9787904),
    (21, 16, 0, 4, 64, 32, 3054080),
    (21, 16, 0, 1, 16, 1201, 17917952),
    (51, 96, 96, 4, 64, 64, 27156992),
    (51, 96, 96, 1, 32, 64, 16712192),
    (51, 96, 96, 1, 32, 3200, 835584512),
    (51, 96, 0, 0, 0, 31, 5582336),
    (51, 96, 0, 4, 64, 1200, 419777024),
    (51, 16, 0, 0, 0, 50, 1743872),
    (51, 16, 0, 1, 32, 1, 1263872),
]


def test_workspace_bytes_unchanged():
    """sd_plan_create needs no device: the size of every recorded (Denoiser, rows) is what it was."""
    lib = _lib.lib()
    for J, D, C, heads, dim_head, rows, want in RECORDED_BYTES:
        d = _lib.SDPlanDesc(num_nodes=J, latent_dim=D, cond_dim=C, out_dim=D, depth=1, attn_heads=heads,
                            attn_dim_head=dim_head, use_attention=int(heads > 0), timesteps=10, isotropic=0, activation=0,
                            sinusoidal_theta=10000.0)
        p = ctypes.c_void_p()
        assert lib.sd_plan_create(ctypes.byref(p), ctypes.byref(d)) == 0, lib.sd_last_error()
        try:
            assert lib.sd_workspace_bytes(p, rows) == want, (J, D, C, heads, dim_head, rows)
        finally:
            lib.sd_plan_destroy(p)
