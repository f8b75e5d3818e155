#!/usr/bin/env python3
"""Generate tests/golden/realism.npz by running the REFERENCE's own body-realism, limb-angle and
CMD functions on the CPU (src/metrics/body_realism.py, src/metrics/multimodal.py:mae,
src/metrics/cmd.py:motion_for_cmd, multimodal.py:cmd).

Build-container tool only, like gen_golden.py: it imports the read-only reference tree (which does
not exist on the GPU box) and no test uses it.  Only reference outputs and the skeletons' integer
limb tables are written; the inputs are regenerated from their seeds by the consumers
(tests/test_metrics_realism.py:_cases restates the recipe below).

Precision.  The inputs are float32 poses, as decoded futures are; the reference's functions are run
on them in float64 (`.double()`), so the fixture holds the exact values of those inputs.  Run in
float32 the reference itself cannot be pinned at the tests' relative tolerance: with reduction
'none' a near-rigid StretchMean entry |mean_len - gt_mean| / gt_mean is a difference of nearly
equal numbers, and float32 rounds it by far more than 1e-5 of its value (this script prints the
reference's own float32-vs-float64 difference per key).

`cmd.py` imports `ignite`, absent here: an empty stub (`Metric`, `NotComputableError`) is registered
in sys.modules first, so the reference's own `motion_for_cmd` runs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_realism.py
"""
from __future__ import annotations

import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SKELDIFF_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

from skeletondiffusion_amd import synthetic  # noqa: E402


def _install_ignite_stub() -> None:
    pkg, met, exc = (types.ModuleType(n) for n in ("ignite", "ignite.metrics", "ignite.exceptions"))
    met.Metric = type("Metric", (), {})
    exc.NotComputableError = type("NotComputableError", (RuntimeError,), {})
    pkg.metrics, pkg.exceptions = met, exc
    sys.modules.update({"ignite": pkg, "ignite.metrics": met, "ignite.exceptions": exc})


_install_ignite_stub()
sys.path.insert(0, REF)
from src.data.skeleton.kinematic import AMASSKinematic, FreeManKinematic, H36MKinematic  # noqa: E402
from src.metrics import body_realism as BR  # noqa: E402
from src.metrics.cmd import motion_for_cmd  # noqa: E402
from src.metrics.multimodal import cmd, mae  # noqa: E402

torch.set_num_threads(8)

# the kinematic classes gen_golden.py constructs (hip excluded, as in eval)
SKELETONS = {
    "h36m16": lambda: H36MKinematic(num_joints=17, if_consider_hip=False),
    "amass21": lambda: AMASSKinematic(num_joints=22, if_consider_hip=False),
    "freeman17": lambda: FreeManKinematic(if_consider_hip=False),
    "mano51": lambda: AMASSKinematic(num_joints=52, if_consider_hip=False),
}


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


def cases():
    """name -> (skeleton, pred (B, S, T, J, 3), target (B, T, J, 3)), float32."""
    rest = N((2, 1, 1, 16, 3), 53) * 0.3
    return {
        "normal": ("h36m16", N((2, 7, 20, 16, 3), 51), N((2, 20, 16, 3), 52)),
        # a near-rigid body: limb lengths move by ~1e-2 around the ground truth's
        "rigid": ("h36m16", rest + 1e-2 * N((2, 7, 20, 16, 3), 54), rest[:, 0] + 1e-3 * N((2, 20, 16, 3), 55)),
        "amass21": ("amass21", N((2, 5, 33, 21, 3), 56), N((2, 33, 21, 3), 57)),
        "mano51": ("mano51", N((1, 3, 4, 51, 3), 58), N((1, 4, 51, 3), 59)),
        "freeman17": ("freeman17", N((1, 2, 5, 17, 3), 60), N((1, 5, 17, 3), 61)),
    }


REDUCTIONS = ("mean", "persample", "none")


def all_metrics(pred, target, limbseq, angles, with_mae=True):
    """Every function x mode x reduction of the new surface, by the reference."""
    out = {}
    for red in REDUCTIONS:
        for mode in ("std", "var"):
            out[f"srmse_{mode}_{red}"] = BR.limb_stretching_normed_rmse(pred, target, limbseq, mode=mode, reduction=red)
            out[f"jrmse_{mode}_{red}"] = BR.limb_jitter_normed_rmse(pred, target, limbseq, mode=mode, reduction=red)
        out[f"smean_{red}"] = BR.limb_stretching_normed_mean(pred, target, limbseq, reduction=red)
        out[f"jmean_{red}"] = BR.limb_jitter_normed_mean(pred, target, limbseq, reduction=red)
    if with_mae:
        out["mae"] = mae(target, pred, limbseq, angles)
        out["mae_cossim"] = mae(target, pred, limbseq, angles, if_return_cossim=True)
    out["motion"] = motion_for_cmd(pred)
    return out


def main():
    arrays, worst = {}, {}
    tables = {}
    for key, ctor in SKELETONS.items():
        sk = ctor()
        limbseq = [[int(a), int(b)] for a, b in sk.get_limbseq()]
        chains = [list(map(int, c)) for c in sk.limb_angles_idx]
        tables[key] = (limbseq, chains)
        arrays[f"{key}_limbseq"] = np.asarray(limbseq, dtype=np.int64)
        arrays[f"{key}_angle_pairs"] = np.asarray([[c[i], c[i + 1]] for c in chains for i in range(len(c) - 1)],
                                                  dtype=np.int64)
        arrays[f"{key}_chain_lengths"] = np.asarray([len(c) for c in chains], dtype=np.int64)

    def record(prefix, pred, target, skel, **kw):
        limbseq, chains = tables[skel]
        r64 = all_metrics(pred.double(), target.double(), limbseq, chains, **kw)
        r32 = all_metrics(pred, target, limbseq, chains, **kw)
        for k, v in r64.items():
            arrays[f"{prefix}_{k}"] = v.numpy()
            a, b = r32[k].double().numpy(), v.numpy()
            ok = np.isfinite(b) & (b != 0)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (prefix, k)
            worst[f"{prefix}_{k}"] = float(np.max(np.abs(a - b)[ok] / np.abs(b)[ok])) if ok.any() else 0.0

    cs = cases()
    for name, (skel, pred, target) in cs.items():
        record(name, pred, target, skel)
    _, pred, target = cs["normal"]
    limbseq, chains = tables["h36m16"]
    record("T2", pred[:, :, :2], target[:, :2], "h36m16")
    record("T1", pred[:, :, :1], target[:, :1], "h36m16")  # jitter: mean of an empty slice -> NaN
    p64, t64 = pred.double(), target.double()
    arrays["normal_mae_t5_15"] = mae(t64, p64, limbseq, chains, t0=5, t=15).numpy()
    arrays["normal_mae_cossim_t5_15"] = mae(t64, p64, limbseq, chains, t0=5, t=15, if_return_cossim=True).numpy()
    obs = N((2, 10, 16, 3), 62)  # a 10-frame observation as the target (config_metrics.py obs_as_target)
    for red in REDUCTIONS:
        arrays[f"normal_smean_obs_{red}"] = BR.limb_stretching_normed_mean(
            p64, obs.double(), limbseq, reduction=red, obs_as_target=True).numpy()
    # cmd of the "normal" case's mean motion profile against a reference motion of 1.5
    profile = motion_for_cmd(p64).mean(0).numpy()
    arrays["cmd_ref"] = np.float64(1.5)
    arrays["cmd_value"] = np.float64(cmd(profile, 1.5))

    print("reference float32 vs float64, max relative difference per key (worst 12):")
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:12]:
        print(f"  {k:32s} {v:.3e}")
    path = os.path.join(HERE, "realism.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
