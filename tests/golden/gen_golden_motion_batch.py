#!/usr/bin/env python3
"""Generate tests/golden/motion_batch.npz by running the REFERENCE's own data path on the CPU:
`MotionDataset.__getitem__` (src/data/loaders/base/motion_dataset.py:184-193) over `BaseDataset.__getitem__`
(base_dataset.py:109-133), with `SkeletonRescalePose` / `SkeletonCenterPose` (src/data/skeleton/motion/).

Build-container tool only, like the other gen_golden_*.py: it imports the read-only reference tree and no test
uses it.  The reference modules are loaded by file under two stub packages, so that their relative imports
resolve without importing the whole data pipeline (`refbase` over loaders/base, `refmot` over skeleton/motion);
they need torch, numpy and scipy.  A three-line MotionDataset subclass fills `annotations`,
`clip_idx_to_metadata` and the generated segments from synthetic clips.

np.random.rand / randint / randn are wrapped, so every draw of the reference is recorded in call order
(base_dataset.py:112 randint; motion_dataset.py:137 rand per mirror axis, :154 rand, :155 randint;
add_noise :15 randn then :16 rand).

Cases (3 ragged clips of 40 / 33 / 57 frames, obs 5, pred 7; every sample_idx of the dataset):
  train_j17 / train_j22 / train_j52   SkeletonRescalePose box 1.5, stride 3, augmentation 2, mirroring 0.5, rotations 0.5
  train_center_j17                    SkeletonCenterPose, same settings
  noisy_j17                           eval, stride 1, if_noisy_obs, noise_level 0.3, noise_std 0.03.  The reference's
                                      add_noise writes into the dataset, so the clips are restored before every item:
                                      each sample is the reference's result on clean data
  segments_j17                        eval, an explicit (clip, init) list in place of the generated one
Stored per case (prefix `<case>_`): clips (F, J, 3) f32 (the clips concatenated) and clip_lengths, segments
(nseg, 3) (clip, init, end), sample_idx, segment_idx, obs, pred, and the recorded draws: offset (B,), mirror (B, 2),
degrees (B,) (-1: none), noise_mask (B, obs, J - 1), noise (B, obs, J - 1, 3) = float32(randn * noise_std).
Data only.

Conditions asserted here: each train case holds >= 8 unrotated samples and >= 8 rotated by an angle that is no
multiple of 90 degrees, its first sample reaches segment 0 and its last one is clamped to the last segment; the
noisy case has hit and unhit pairs in every sample.  The numpy seed of a case is the first one that meets them.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_motion_batch.py
"""
from __future__ import annotations

import importlib
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SKELDIFF_REFERENCE", "/root/reference")

for name, rel in (("refbase", "src/data/loaders/base"), ("refmot", "src/data/skeleton/motion")):
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(REF, rel)]
    sys.modules[name] = pkg
motion_dataset = importlib.import_module("refbase.motion_dataset")
rescalepose = importlib.import_module("refmot.rescalepose")
centerpose = importlib.import_module("refmot.centerpose")

LENGTHS, OBS, PRED = (40, 33, 57), 5, 7
SEG = OBS + PRED


class _Dataset(motion_dataset.MotionDataset):
    def _prepare_data(self, num_workers=8):
        self.mm_indces = None  # as the reference's datasets set it in _prepare_data (no multimodal GT loaded)
        self.annotations = [c.copy() for c in self.skeleton.clips]
        self.clip_idx_to_metadata = [("subject", f"action{i}") for i in range(len(self.annotations))]
        self.segments, self.segment_idx_to_metadata = self._generate_segments()


class _Recorder:
    """np.random.rand / randint / randn replaced by wrappers that log (name, value) in call order."""

    def __enter__(self):
        self.log = []
        self.saved = {n: getattr(np.random, n) for n in ("rand", "randint", "randn")}
        for n, f in self.saved.items():
            setattr(np.random, n, self._wrap(n, f))
        return self

    def _wrap(self, name, f):
        def g(*a, **k):
            v = f(*a, **k)
            self.log.append((name, v))
            return v
        return g

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(np.random, n, f)


def make_clips(J, seed):
    """A wandering hip plus a fixed pose and small per-frame motion: |coordinate| up to ~3."""
    rs = np.random.RandomState(seed)
    clips = []
    for T in LENGTHS:
        hip = np.cumsum(rs.randn(T, 1, 3) * 0.05, 0) + rs.uniform(-2, 2, (1, 1, 3))
        pose = rs.uniform(-0.9, 0.9, (1, J, 3))
        pose[:, 0] = 0
        clips.append((hip + pose + rs.randn(T, J, 3) * 0.02).astype(np.float32))
    return clips


def make_dataset(clips, cls, split, tmp, **kw):
    skeleton = cls(if_consider_hip=False, obs_length=OBS, pred_length=PRED, **({"pose_box_size": 1.5} if cls is rescalepose.SkeletonRescalePose else {}))
    skeleton.clips, skeleton.adj_matrix, skeleton.num_joints = clips, None, clips[0].shape[1]
    return _Dataset(split, tmp, skeleton, OBS, PRED, dtype="float32", if_consider_hip=False, silent=True, **kw)


def run(ds, clips, numpy_seed, noisy):
    """Every sample of the dataset once; the draws parsed from the recorder's log."""
    J, B = clips[0].shape[1], len(ds)
    out = dict(offset=np.zeros(B, np.int32), mirror=np.zeros((B, 2), bool), degrees=np.full(B, -1, np.int32),
               noise_mask=np.zeros((B, OBS, J - 1), bool), noise=np.zeros((B, OBS, J - 1, 3), np.float32),
               obs=np.zeros((B, OBS, J - 1, 3), np.float32), pred=np.zeros((B, PRED, J - 1, 3), np.float32),
               segment_idx=np.zeros(B, np.int64), sample_idx=np.arange(B, dtype=np.int64))
    np.random.seed(numpy_seed)
    for b in range(B):
        ds.annotations = [c.copy() for c in clips]  # add_noise writes into the dataset: start every item clean
        with _Recorder() as rec:
            obs, pred, extra = ds[b]
        log = list(rec.log)
        if ds.augmentation != 0:
            name, v = log.pop(0)
            assert name == "randint"
            out["offset"][b] = v
        if noisy:
            (n1, z), (n2, u) = log.pop(0), log.pop(0)
            assert n1 == "randn" and n2 == "rand" and z.shape == (OBS, J - 1, 3) and u.shape == (OBS, J - 1)
            out["noise"][b] = (z * ds.noise_std).astype(np.float32)
            out["noise_mask"][b] = u < ds.noise_level
        if not ds.in_eval:
            if ds.da_mirroring != 0:
                for m in (0, 1):
                    name, v = log.pop(0)
                    assert name == "rand"
                    out["mirror"][b, m] = v < ds.da_mirroring
            if ds.da_rotations != 0:
                name, v = log.pop(0)
                assert name == "rand"
                if v < ds.da_rotations:
                    name, d = log.pop(0)
                    assert name == "randint"
                    out["degrees"][b] = d
        assert not log, log
        assert obs.dtype == torch.float32 and extra["sample_idx"] == b
        out["obs"][b], out["pred"][b], out["segment_idx"][b] = obs.numpy(), pred.numpy(), extra["segment_idx"]
    return out


def store(z, case, clips, ds, out):
    z[f"{case}_clips"] = np.concatenate(clips, 0)
    z[f"{case}_clip_lengths"] = np.asarray([len(c) for c in clips], np.int64)
    z[f"{case}_segments"] = np.asarray(ds.segments, np.int64).reshape(-1, 3)
    for k, v in out.items():
        z[f"{case}_{k}"] = v


def main():
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        train = dict(stride=3, augmentation=2, da_mirroring=0.5, da_rotations=0.5)
        for case, J, cls in (("train_j17", 17, rescalepose.SkeletonRescalePose), ("train_j22", 22, rescalepose.SkeletonRescalePose),
                             ("train_j52", 52, rescalepose.SkeletonRescalePose), ("train_center_j17", 17, centerpose.SkeletonCenterPose)):
            clips = make_clips(J, 100 + J)
            ds = make_dataset(clips, cls, "train", tmp, **train)
            nseg = len(ds.segments)
            assert nseg == sum(T - SEG for T in LENGTHS) and len(ds) == nseg // 3
            for numpy_seed in range(10000):
                out = run(ds, clips, numpy_seed, False)
                deg = out["degrees"]
                raw_last = 3 * (len(ds) - 1) + 2 + out["offset"][-1]
                if (deg < 0).sum() >= 8 and ((deg >= 0) & (deg % 90 != 0)).sum() >= 8 and out["segment_idx"][0] == 0 and \
                        raw_last > nseg - 1 and out["segment_idx"][-1] == nseg - 1:
                    break
            else:
                raise AssertionError("no seed meets the conditions")
            print(f"{case}: numpy seed {numpy_seed}, {len(ds)} samples, {(deg < 0).sum()} unrotated, "
                  f"{((deg >= 0) & (deg % 90 != 0)).sum()} rotated off the axes, max |raw| {np.abs(np.concatenate(clips)).max():.3f}")
            store(z, case, clips, ds, out)
            z[f"{case}_numpy_seed"] = np.int64(numpy_seed)

        clips = make_clips(17, 117)
        ds = make_dataset(clips, rescalepose.SkeletonRescalePose, "valid", tmp, stride=1, augmentation=0, if_noisy_obs=True,
                          noise_level=0.3, noise_std=0.03)
        assert ds.in_eval
        out = run(ds, clips, 7, True)
        per = out["noise_mask"].reshape(len(ds), -1)
        assert (per.any(1) & ~per.all(1)).all(), "a sample without both hit and unhit pairs"
        print(f"noisy_j17: {len(ds)} samples, hit share {per.mean():.3f}")
        store(z, "noisy_j17", clips, ds, out)

        ds = make_dataset(clips, rescalepose.SkeletonRescalePose, "valid", tmp, stride=1, augmentation=0)
        rs = np.random.RandomState(5)
        listed = [(c, int(i)) for c, T in enumerate(LENGTHS) for i in sorted(rs.choice(T - SEG + 1, 6, replace=False))]
        listed += [(c, T - SEG) for c, T in enumerate(LENGTHS) if (c, T - SEG) not in listed]  # the last possible start
        ds.segments = [(c, i, i + SEG - 1) for c, i in listed]
        ds.segment_idx_to_metadata = [ds.clip_idx_to_metadata[c] for c, _ in listed]
        out = run(ds, clips, 0, False)
        assert (out["segment_idx"] == np.arange(len(listed))).all()
        print(f"segments_j17: {len(ds)} listed segments")
        store(z, "segments_j17", clips, ds, out)

    path = os.path.join(HERE, "motion_batch.npz")
    np.savez_compressed(path, obs_length=np.int64(OBS), pred_length=np.int64(PRED), **z)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
