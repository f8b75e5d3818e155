"""Host side of the on-device body-realism / limb-angle / motion-profile metrics: the
public surface, the C ABI and its argument checks, the limb tables, and a stand-alone emulation of the
kernels' address arithmetic under AddressSanitizer.  No GPU; the device parity tests are in
tests/test_gpu_realism.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from skeletondiffusion_amd import _lib
from test_metrics_realism import _tables

SKELETONS = ("h36m16", "amass21", "freeman17", "mano51")
NAMES = ("limb_stretching_normed_rmse", "limb_stretching_normed_mean", "limb_jitter_normed_rmse",
         "limb_jitter_normed_mean", "mae", "motion_for_cmd", "realism")


def test_public_surface_refuses_cpu_tensors():
    from skeletondiffusion_amd import metrics as M, skeletons
    from skeletondiffusion_amd._lib import SkelDiffError

    for name in NAMES:
        assert name in M.__all__ and callable(getattr(M, name)), name
    pred, target = torch.zeros(2, 3, 4, 16, 3), torch.zeros(2, 4, 16, 3)
    ls, chains = skeletons.limbseq("h36m16"), skeletons.limb_angles_idx("h36m16")
    for fn in (M.limb_stretching_normed_rmse, M.limb_stretching_normed_mean, M.limb_jitter_normed_rmse,
               M.limb_jitter_normed_mean, M.realism):
        with pytest.raises(SkelDiffError):
            fn(pred, target, ls)
    with pytest.raises(SkelDiffError):
        M.realism(pred, target, ls, chains)
    with pytest.raises(SkelDiffError):
        M.mae(target, pred, ls, chains)
    with pytest.raises(SkelDiffError):
        M.motion_for_cmd(pred)


def test_stats_funcs_have_the_reference_key_sets():
    """src/config_metrics.py:30-50."""
    from skeletondiffusion_amd import evaluation as E

    realism = {"StretchMean", "JitterMean", "StretchRMSE", "JitterRMSE"}
    assert "get_stats_funcs" in E.__all__
    for skel in SKELETONS:
        assert set(E.get_stats_funcs("deterministic", skel)) == {"ADE", "FDE", "MAE", "APD"} | realism
        assert set(E.get_stats_funcs("probabilistic_orig", skel)) == {"APD", "ADE", "FDE", "MMADE", "MMFDE"}
        assert set(E.get_stats_funcs("probabilistic", skel)) == {"ADE", "FDE", "MAE", "MMADE", "MMFDE", "APD"} | realism
    funcs = E.get_stats_funcs("probabilistic", "amass21")
    assert all(callable(f) for f in funcs.values())
    with pytest.raises(NotImplementedError):
        E.get_stats_funcs("other", "amass21")


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bint sd_realism_target\(const float\* target, int64_t nseq", hdr)
    assert re.search(r"\bint sd_realism\(const float\* pred, int64_t nseq", hdr)
    assert re.search(r"\bint32_t sd_realism_frame_tile\(int32_t joints\)", hdr)
    for name in ("sd_realism_target", "sd_realism", "sd_realism_frame_tile"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4


def _i32(rows):
    flat = [int(v) for r in rows for v in r]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat)


def test_host_argument_checks():
    """sd_realism / sd_realism_target validate on the host, before any device call, and name the argument."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)
    limbs3 = [[0, 1], [1, 2], [2, 3]]

    def pred_call(nseq=2, samples=5, frames=7, joints=4, limbs=limbs3, nlimbs=None, pairs=((0, 1),), npairs=None,
                  target_frames=7, angle=None):
        return L.sd_realism(p, nseq, samples, frames, joints, _i32(limbs), len(limbs) if nlimbs is None else nlimbs,
                            _i32(pairs), len(pairs) if npairs is None else npairs, p, p, p, target_frames, None, p, None,
                            None, angle, None, None, None, None, None, None)

    def target_call(nseq=2, frames=7, joints=4, limbs=limbs3, nlimbs=None, pairs=((0, 1),), npairs=None):
        return L.sd_realism_target(p, nseq, frames, joints, _i32(limbs), len(limbs) if nlimbs is None else nlimbs,
                                   _i32(pairs), len(pairs) if npairs is None else npairs, p, None, None, None)

    common = ((dict(frames=0), b"frames"), (dict(joints=0), b"joints"), (dict(joints=65), b"joints"),
              (dict(nlimbs=0), b"nlimbs"), (dict(nlimbs=65, limbs=[[0, 1]] * 65), b"nlimbs"),
              (dict(npairs=65, pairs=[[0, 1]] * 65), b"npairs"),
              (dict(limbs=[[0, 1], [1, 4], [2, 3]]), b"limbseq[1]"), (dict(limbs=[[-1, 1], [1, 2], [2, 3]]), b"limbseq[0]"),
              (dict(pairs=[[0, 1], [1, 3]]), b"angle_pairs[1]"), (dict(pairs=[[-1, 1]]), b"angle_pairs[0]"))
    for call, cases in ((pred_call, common + ((dict(samples=0), b"samples"), (dict(samples=65), b"samples"),
                                              (dict(target_frames=6, angle=p), b"target_frames"))),
                        (target_call, common)):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())
    assert L.sd_realism(None, 0, 5, 7, 4, _i32(limbs3), 3, None, 0, None, None, None, 7, *([None] * 11)) == 0
    assert L.sd_realism_target(None, 0, 7, 4, _i32(limbs3), 3, None, 0, None, None, None, None) == 0
    for joints, tile in ((16, 32), (21, 32), (17, 32), (51, 13), (64, 10), (1, 32)):
        assert L.sd_realism_frame_tile(joints) == tile
    assert L.sd_realism_frame_tile(0) == -1 and L.sd_realism_frame_tile(65) == -1


def test_limb_tables_equal_the_fixture():
    from skeletondiffusion_amd import skeletons

    z = golden("realism")
    for skel in SKELETONS:
        limbseq, chains = _tables(z, skel)
        assert skeletons.limbseq(skel) == limbseq, skel  # in order: the chains index into it
        assert skeletons.limb_angles_idx(skel) == chains, skel
        assert np.array_equal(np.asarray(skeletons.limbseq(skel)), z[f"{skel}_limbseq"])
    with pytest.raises(KeyError):
        skeletons.limbseq("mano52")


def test_kernel_addresses_in_bounds_under_asan(tmp_path):
    """tests/host/realism_emulation.cpp walks every workgroup x thread x load / store of the three kernels
    with the kernels' own address functions (csrc/sd_realism_addr.h): on real heap buffers at the
    fixture's shapes under AddressSanitizer + UBSan, arithmetically at 8 and 256 x 50 x 120 x 21 x 3."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "realism_emulation")
    src = os.path.join(REPO, "tests", "host", "realism_emulation.cpp")
    # the sanitizer runtime is linked statically (g++ -static-libasan; clang's default), so the program
    # needs nothing preloaded and does not mind what its environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "realism emulation ok" in r.stdout
