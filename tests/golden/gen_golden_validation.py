#!/usr/bin/env python3
"""Generate tests/golden/validation.npz by running the REFERENCE's own validation metrics on the CPU:
src/metrics/body_realism.py:4-107 (limb_length_variance, limb_length_jitter, limb_length_error,
limb_length_variation_difference_wrtGT), src/metrics/ignite_mpjpe.py (MeanPerJointPositionError),
src/metrics/ignite_fde.py (FinalDisplacementError) and src/metrics/utils.py (choose_best_sample,
format_metric_time_table).

Build-container tool only, like gen_golden_realism.py: it imports the read-only reference tree (which
does not exist on the GPU box) and no test uses it.  Only reference outputs and the skeletons' integer
limb tables are written; the inputs are regenerated from their seeds by the consumers
(tests/test_validation_metrics.py restates the recipe below).

Precision.  The inputs are float32 poses; the reference's functions and metric classes are run on them
in float64 (`.double()`), so the fixture holds the exact values of those inputs.  The script prints the
reference's own float32-vs-float64 difference per key: on the near-rigid case its float32 variance is
off by far more than the tests' relative tolerance.  The (B, S, T - 1, L) arrays of mode 'none' are
stored as the float32 rounding of the float64 result (6e-8 of each value, the tolerance is 1e-5), which
keeps the file the size of realism.npz.

`ignite` is absent here: a stub is registered in sys.modules first whose `Metric` has the two things
the metric classes use, `__init__(self, output_transform=...)` and `reset`.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_validation.py
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


class _Metric:
    def __init__(self, output_transform=lambda x: x, **kwargs):
        self._output_transform = output_transform
        self.reset()

    def reset(self):
        pass


def _install_ignite_stub() -> None:
    pkg, met, exc = (types.ModuleType(n) for n in ("ignite", "ignite.metrics", "ignite.exceptions"))
    met.Metric = _Metric
    exc.NotComputableError = type("NotComputableError", (RuntimeError,), {})
    pkg.metrics, pkg.exceptions = met, exc
    sys.modules.update({"ignite": pkg, "ignite.metrics": met, "ignite.exceptions": exc})


_install_ignite_stub()
sys.path.insert(0, REF)
from src.data.skeleton.kinematic import AMASSKinematic, FreeManKinematic, H36MKinematic  # noqa: E402
from src.metrics import body_realism as BR  # noqa: E402
from src.metrics.ignite_fde import FinalDisplacementError  # noqa: E402
from src.metrics.ignite_mpjpe import MeanPerJointPositionError  # noqa: E402
from src.metrics.utils import choose_best_sample  # noqa: E402

torch.set_num_threads(8)

SKELETONS = {
    "h36m16": lambda: H36MKinematic(num_joints=17, if_consider_hip=False),
    "amass21": lambda: AMASSKinematic(num_joints=22, if_consider_hip=False),
    "freeman17": lambda: FreeManKinematic(if_consider_hip=False),
    "mano51": lambda: AMASSKinematic(num_joints=52, if_consider_hip=False),
}
MODES = ("mean", "max", "min", "none")
LONG_BATCHES = (5, 2, 4)  # the long case's rows, fed to the metric classes in three uneven batches


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


def cases():
    """name -> (skeleton, pred (B, S, T, J, 3), target (B, T, J, 3)), float32: the realism recipe's."""
    rest = N((2, 1, 1, 16, 3), 53) * 0.3
    c = {
        "normal": ("h36m16", N((2, 7, 20, 16, 3), 51), N((2, 20, 16, 3), 52)),
        # a near-rigid body: limb lengths move by ~1e-2 around the ground truth's
        "rigid": ("h36m16", rest + 1e-2 * N((2, 7, 20, 16, 3), 54), rest[:, 0] + 1e-3 * N((2, 20, 16, 3), 55)),
        "amass21": ("amass21", N((2, 5, 33, 21, 3), 56), N((2, 33, 21, 3), 57)),
        "mano51": ("mano51", N((1, 3, 4, 51, 3), 58), N((1, 4, 51, 3), 59)),
        "freeman17": ("freeman17", N((1, 2, 5, 17, 3), 60), N((1, 5, 17, 3), 61)),
    }
    _, pred, target = c["normal"]
    c["T2"] = ("h36m16", pred[:, :, :2], target[:, :2])
    c["T1"] = ("h36m16", pred[:, :, :1], target[:, :1])
    return c


def long_case():
    """(pred (11, 3, 61, 16, 3), target (11, 61, 16, 3)): the time table has rows 0, 30, 60."""
    rows = sum(LONG_BATCHES)
    return N((rows, 3, 61, 16, 3), 63), N((rows, 61, 16, 3), 64)


def all_metrics(pred, target, limbseq):
    """Every function x mode x if_per_sample of the new surface, by the reference; where it raises (max / min
    of the jitter of a single frame) the key is absent."""
    out = {}
    for mode in MODES:
        for ps in (False, True):
            if mode == "none" and ps:
                continue  # if_per_sample is not read on this branch
            tag = f"{mode}_ps" if ps else mode
            out[f"variance_{tag}"] = BR.limb_length_variance(pred, limbseq, mode=mode, if_per_sample=ps)
            try:
                out[f"jitter_{tag}"] = BR.limb_length_jitter(pred, limbseq, mode=mode, if_per_sample=ps)
            except (RuntimeError, IndexError):
                assert pred.shape[2] == 1 and mode in ("max", "min")
        if mode != "none":
            out[f"error_{mode}"] = BR.limb_length_error(target, pred, limbseq, mode=mode)
        try:
            out[f"wrtgt_{mode}"] = BR.limb_length_variation_difference_wrtGT(target, pred, limbseq, mode=mode)
        except (RuntimeError, IndexError):
            assert pred.shape[2] == 1 and mode in ("max", "min")
    return out


def frame_metrics(pred, target):
    """The metric classes fed in LONG_BATCHES: the profile of sample 0 and of the best sample, the FDE."""
    out = {}

    def run(metric, transform):
        metric.reset()
        r0 = 0
        for n in LONG_BATCHES:
            metric.update(transform(pred[r0:r0 + n], target[r0:r0 + n]))
            r0 += n
        return metric.compute()

    first = lambda p, t: (p[:, 0], t)  # noqa: E731
    out["long_mpjpe_table"] = run(MeanPerJointPositionError(), first)
    out["long_mpjpe_joint_table"] = run(MeanPerJointPositionError(keep_joint_dim=True), first)
    out["long_mpjpe_mean"] = run(MeanPerJointPositionError(keep_time_dim=False), first)
    out["long_mpjpe_joint_mean"] = run(MeanPerJointPositionError(keep_time_dim=False, keep_joint_dim=True), first)
    out["long_fde"] = run(FinalDisplacementError(), first)
    out["long_best_mpjpe_table"] = run(MeanPerJointPositionError(), choose_best_sample)
    out["long_best_fde"] = run(FinalDisplacementError(), choose_best_sample)
    return out


def main():
    arrays, worst = {}, {}

    def record(r64, r32, prefix=""):
        for k, v in r64.items():
            key = prefix + k
            b = v.numpy()
            arrays[key] = b.astype(np.float32) if b.ndim == 4 else b
            a = r32[k].double().numpy()
            ok = np.isfinite(b) & (b != 0)
            assert np.array_equal(np.isnan(a), np.isnan(b)), key
            worst[key] = float(np.max(np.abs(a - b)[ok] / np.abs(b)[ok])) if ok.any() else 0.0

    for name, (skel, pred, target) in cases().items():
        limbseq = [[int(a), int(b)] for a, b in SKELETONS[skel]().get_limbseq()]
        arrays[f"{skel}_limbseq"] = np.asarray(limbseq, dtype=np.int64)
        record(all_metrics(pred.double(), target.double(), limbseq), all_metrics(pred, target, limbseq), name + "_")
    pred, target = long_case()
    record(frame_metrics(pred.double(), target.double()), frame_metrics(pred, target))
    arrays["long_batches"] = np.asarray(LONG_BATCHES, dtype=np.int64)

    print("reference float32 vs float64, max relative difference per key (worst 12):")
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:12]:
        print(f"  {k:32s} {v:.3e}")
    path = os.path.join(HERE, "validation.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
