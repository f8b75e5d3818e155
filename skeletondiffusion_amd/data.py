"""Motion batches on the device: the reference's data path without a host loader.

    DeviceMotionData(clips, obs_length, pred_length, ...)   the clips of a split, resident on the device
        .batch(sample_idx, train=...)     obs, pred, extra of those samples: one kernel (sd_motion_batch)
        .draws(sample_idx, seed, epoch)   the random decisions `batch` takes from the Philox stream, as tensors
        .batches(batch_size, ...)         an epoch of batches over a device randperm
        .all_futures() / .last_obs()      every segment's future / last observed frame, unaugmented
    MotionRepresentation                  tranform_to_input_space / transform_to_metric_space /
                                          if_add_zero_pad_center_hip of the reference's three skeleton
                                          classes, as torch ops on any device

Per sample it computes what `MotionDataset.__getitem__` (src/data/loaders/base/motion_dataset.py:184-193) over
`BaseDataset.__getitem__` (base_dataset.py:109-133) does: the segment with its augmentation offset and clamp,
`add_noise` on the observation, mirroring and the rotation about z, then `Skeleton.tranform_to_input_space`
with `if_consider_hip=False`.  `default_collate` and the host-to-device copy have no counterpart: the batch is
written where it is used.  Batches are built on ROCm tensors only (no CPU path); the segment table,
`__len__` and `MotionRepresentation` need no device.

Random decisions come from the sampler's Philox stream keyed (seed, row = sample_idx, step = epoch): what a
sample gets does not depend on its batch-mates or its position.  `draws=` replaces them with given ones
(`draws()` output, or the recorded draws of a run of the reference).

Deliberate differences from the reference:
  * The reference's `add_noise` writes into a view of `self.annotations`, so its noise accumulates in the
    dataset from epoch to epoch.  The resident clips here are never written: every batch starts from clean data.
  * `if_consider_hip=True` raises AttributeError in the reference (base.py:22-31 defines
    `_get_where_is_seq_centered` as a nested function and calls it as a method).  It is refused by name.
  * `SkeletonDiscreteCosineTransform`, `normalize_data` and float64 clips are refused by name.
  * The training-time `mm_gt` augmentation (`if_load_mmgt`) is not built.
  * The rotation uses c, s = float32(cos), float32(sin) of the float64 angle, not scipy's quaternion route to
    the matrix: the entries differ by a rounding at most.
  * Random numbers are Philox, not numpy's Mersenne twister; a numpy run is replayed through `draws=`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import SkelDiffError, check

REPRESENTATIONS = {"SkeletonVanilla": _lib.SD_MOTION_VANILLA, "SkeletonCenterPose": _lib.SD_MOTION_CENTER_POSE,
                   "SkeletonRescalePose": _lib.SD_MOTION_RESCALE_POSE}


def _representation(motion_repr_type: str) -> int:
    if motion_repr_type not in REPRESENTATIONS:
        raise SkelDiffError(f"motion_repr_type {motion_repr_type!r} is not supported (SkeletonDiscreteCosineTransform among "
                            f"them): one of {sorted(REPRESENTATIONS)}")
    return REPRESENTATIONS[motion_repr_type]


def _refuse(if_consider_hip=False, normalize_data=False, **unknown) -> None:
    if if_consider_hip:
        raise SkelDiffError("if_consider_hip=True is not supported (the reference raises AttributeError there, base.py:22-31)")
    if normalize_data:
        raise SkelDiffError("normalize_data=True is not supported (the reference asserts it off, base_dataset.py:56)")
    if unknown:
        raise TypeError(f"unexpected arguments {sorted(unknown)}")


def generate_segments(lengths, seg_length: int) -> np.ndarray:
    """base_dataset.py:189-198: (clip, init) for init in range(0, T_i - seg_length), clips in order, as an
    (nseg, 2) int64 array.  The range leaves out the last possible start, as the reference's does."""
    rows = [(i, init) for i, T in enumerate(lengths) for init in range(0, int(T) - seg_length)]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 2)


def segment_index(sample_idx, offset, stride: int, augmentation: int, nseg: int) -> np.ndarray:
    """base_dataset.py:110-113 on host arrays, clamped to [0, nseg - 1] as the kernel clamps it."""
    s = stride * np.asarray(sample_idx, dtype=np.int64) + augmentation
    if augmentation != 0:
        s = s + np.asarray(offset, dtype=np.int64)
    return np.clip(s, 0, nseg - 1)


def rotation_table() -> np.ndarray:
    """(720,) float32: the float32 roundings of the float64 cosines of 0..359 degrees, then of the sines."""
    rad = np.deg2rad(np.arange(360, dtype=np.float64))
    return np.concatenate([np.cos(rad), np.sin(rad)]).astype(np.float32)


class MotionRepresentation:
    """The reference's SkeletonVanilla / SkeletonCenterPose / SkeletonRescalePose (src/data/skeleton/motion/) with
    if_consider_hip=False, as torch ops on any device: data (..., J_full, 3) -> input space (..., J_full - 1, 3)
    and back to metric space."""

    def __init__(self, motion_repr_type: str = "SkeletonRescalePose", num_joints: int = None, pose_box_size: float = 1.5,
                 **kwargs):
        _refuse(**kwargs)
        self.repr = _representation(motion_repr_type)
        self.motion_repr_type = motion_repr_type
        self.num_joints = num_joints
        self.pose_box_size = float(pose_box_size)
        self.if_consider_hip = False
        if not self.pose_box_size > 0:
            raise ValueError("pose_box_size must be > 0")

    def tranform_to_input_space(self, data: torch.Tensor) -> torch.Tensor:
        """base.py:35-42 (the reference's spelling)."""
        if self.repr == _lib.SD_MOTION_VANILLA:
            return data[..., 1:, :]
        centered = (data - data[..., 0:1, :])[..., 1:, :]
        if self.repr == _lib.SD_MOTION_RESCALE_POSE:
            # a tensor divisor on the data's device: a true division on every backend (a Python scalar may
            # be turned into a multiplication by its reciprocal)
            centered = centered / torch.tensor(self.pose_box_size, dtype=data.dtype, device=data.device)
        return centered

    def transform_to_metric_space(self, kpts: torch.Tensor) -> torch.Tensor:
        """base.py:69-86: the hip-centred pose in metric units."""
        if self.repr == _lib.SD_MOTION_RESCALE_POSE:
            return kpts * self.pose_box_size
        return kpts

    def add_zero_pad_center_hip(self, kpts: torch.Tensor) -> torch.Tensor:
        shape = list(kpts.shape)
        shape[-2] = 1
        return torch.cat([torch.zeros(shape, device=kpts.device, dtype=kpts.dtype), kpts], dim=-2)

    def if_add_zero_pad_center_hip(self, kpts: torch.Tensor) -> torch.Tensor:
        """base.py:54-57."""
        if self.num_joints is not None and kpts.shape[-2] == self.num_joints - 1:
            kpts = self.add_zero_pad_center_hip(kpts)
        return kpts


class DeviceMotionData:
    def __init__(self, clips, obs_length: int, pred_length: int, *, stride: int = 1, augmentation: int = 0,
                 da_mirroring: float = 0.0, da_rotations: float = 0.0, if_noisy_obs: bool = False, noise_level: float = 0.30,
                 noise_std: float = 0.03, motion_repr_type: str = "SkeletonRescalePose", pose_box_size: float = 1.5,
                 clip_class=None, segments=None, device="cuda", **kwargs):
        _refuse(**kwargs)
        self.repr = _representation(motion_repr_type)
        if obs_length < 1 or pred_length < 1:
            raise ValueError("obs_length and pred_length must be >= 1")
        if augmentation < 0:
            raise ValueError("augmentation must be >= 0")
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if not (0.0 <= da_mirroring <= 1.0 and 0.0 <= da_rotations <= 1.0 and 0.0 <= noise_level <= 1.0):
            raise ValueError("da_mirroring, da_rotations and noise_level must be in [0, 1]")
        if not pose_box_size > 0:
            raise ValueError("pose_box_size must be > 0")
        host = []
        for i, c in enumerate(clips):
            c = c.detach().cpu() if torch.is_tensor(c) else torch.from_numpy(np.asarray(c))
            if c.dtype == torch.float64:
                raise SkelDiffError(f"clips[{i}] is float64: float64 data is not supported, pass float32 (the release "
                                    "configs' dtype)")
            if c.dtype != torch.float32 or c.dim() != 3 or c.shape[2] != 3:
                raise ValueError(f"clips[{i}]: a (T, J_full, 3) float32 array expected, got {c.dtype} {tuple(c.shape)}")
            host.append(c)
        if not host:
            raise ValueError("clips is empty")
        self.num_joints = int(host[0].shape[1])
        if any(c.shape[1] != self.num_joints for c in host):
            raise ValueError("clips differ in their joint count")
        if not 2 <= self.num_joints <= 64:
            raise ValueError("J_full must be in [2, 64]")
        self.obs_length, self.pred_length = int(obs_length), int(pred_length)
        self.seg_length = self.obs_length + self.pred_length
        lengths = [int(c.shape[0]) for c in host]
        clip_first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        if segments is not None:  # h36m.py:37-40: a test split read from its CSV
            seg = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
            stride, augmentation = 1, 0
            for k, (ci, init) in enumerate(seg.tolist()):
                if not (0 <= ci < len(host) and 0 <= init and init + self.seg_length <= lengths[ci]):
                    raise ValueError(f"segments[{k}] = ({ci}, {init}) does not lie inside its clip")
        else:
            seg = generate_segments(lengths, self.seg_length)
        if len(seg) < 1:
            raise ValueError("no clip is longer than obs_length + pred_length: there are no segments")
        self.stride, self.augmentation = int(stride), int(augmentation)
        self.da_mirroring, self.da_rotations = float(da_mirroring), float(da_rotations)
        self.if_noisy_obs, self.noise_level, self.noise_std = bool(if_noisy_obs), float(noise_level), float(noise_std)
        self.motion_repr_type, self.pose_box_size = motion_repr_type, float(pose_box_size)
        self.representation = MotionRepresentation(motion_repr_type, self.num_joints, pose_box_size)
        self.segments = seg  # host (nseg, 2) int64: (clip, init)
        self.nseg = int(len(seg))
        self.device = torch.device(device)
        # resident tensors
        self.frames = torch.cat(host, 0).contiguous().to(self.device)  # (F, J_full, 3) f32
        self.total_frames = int(self.frames.shape[0])
        self.seg_first = torch.from_numpy(clip_first[seg[:, 0]] + seg[:, 1]).to(self.device)  # (nseg,) int64
        self.seg_clip = torch.from_numpy(np.ascontiguousarray(seg[:, 0])).to(self.device)
        self.seg_init = torch.from_numpy(np.ascontiguousarray(seg[:, 1])).to(self.device)
        self.clip_class = None
        if clip_class is not None:
            cc = torch.as_tensor(clip_class, dtype=torch.int64).reshape(-1)
            if cc.numel() != len(host):
                raise ValueError("clip_class needs one entry per clip")
            self.clip_class = cc.to(self.device)
        self.rot_table = torch.from_numpy(rotation_table()).to(self.device)

    def __len__(self) -> int:
        return self.nseg // self.stride

    # ---- launches --------------------------------------------------------------------------------------------
    def _require_device(self) -> None:
        if self.device.type != "cuda":
            raise SkelDiffError("DeviceMotionData: batches are built on the MI355X HIP engine only; construct it with a ROCm "
                                "device")

    def _index(self, sample_idx) -> torch.Tensor:
        if torch.is_tensor(sample_idx) and sample_idx.device.type == "cuda":
            return sample_idx.detach().to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        idx = torch.as_tensor(sample_idx, dtype=torch.int64).reshape(-1)  # host: checked here
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"sample_idx outside 0..{len(self) - 1}")
        return idx.to(self.device)

    def _launch(self, idx, train, seed, epoch, draws, stride, augmentation, noisy):
        B, J, dev = idx.numel(), self.num_joints, self.device
        obs = torch.empty(B, self.obs_length, J - 1, 3, device=dev, dtype=torch.float32)
        pred = torch.empty(B, self.pred_length, J - 1, 3, device=dev, dtype=torch.float32)
        seg = torch.empty(B, device=dev, dtype=torch.int64)
        d = [None] * 5
        keep = []
        if draws is not None:
            def arg(name, shape, dtype, fill):
                t = draws.get(name)
                if t is None:
                    t = torch.full(shape, fill, dtype=dtype, device=dev)
                t = torch.as_tensor(t).to(device=dev, dtype=dtype).contiguous()
                if tuple(t.shape) != tuple(shape):
                    raise ValueError(f"draws[{name!r}]: shape {tuple(shape)} expected, got {tuple(t.shape)}")
                keep.append(t)
                return t.data_ptr() if t.numel() else None
            d[0] = arg("offset", (B,), torch.int32, 0)
            d[1] = arg("mirror", (B, 2), torch.uint8, 0)
            d[2] = arg("degrees", (B,), torch.int32, -1)
            if noisy:
                d[3] = arg("noise_mask", (B, self.obs_length, J - 1), torch.uint8, 0)
                d[4] = arg("noise", (B, self.obs_length, J - 1, 3), torch.float32, 0.0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(_lib.lib().sd_motion_batch(
            self.frames.data_ptr(), self.total_frames, self.seg_first.data_ptr(), self.nseg, idx.data_ptr() if B else None, B,
            J, self.obs_length, self.pred_length, stride, augmentation, int(bool(train)), self.repr, self.pose_box_size,
            self.da_mirroring, self.da_rotations, int(noisy), self.noise_level, self.noise_std, self.rot_table.data_ptr(),
            int(seed) & (2 ** 64 - 1), int(epoch), *d, obs.data_ptr() if B else None, pred.data_ptr() if B else None,
            seg.data_ptr() if B else None, stream))
        return obs, pred, seg

    def batch(self, sample_idx, *, train: bool, seed=None, epoch: int = 0, draws=None):
        """obs (B, obs_length, J_full - 1, 3), pred (B, pred_length, J_full - 1, 3), extra.  sample_idx: a list or
        host tensor (checked against len(self)) or a device int64 tensor (not checked: no host synchronisation).
        train=False leaves out the mirroring and the rotation; the segment offset and the observation noise
        apply in both modes, as in the reference.  Work goes on torch's current stream."""
        self._require_device()
        idx = self._index(sample_idx)
        obs, pred, seg = self._launch(idx, train, 0 if seed is None else seed, epoch, draws, self.stride, self.augmentation,
                                      self.if_noisy_obs)
        init = self.seg_init.index_select(0, seg)
        clip = self.seg_clip.index_select(0, seg)
        extra = {"sample_idx": idx, "segment_idx": seg, "clip_idx": clip, "init": init, "end": init + (self.seg_length - 1)}
        if self.clip_class is not None:
            extra["class_idx"] = self.clip_class.index_select(0, clip)
        return obs, pred, extra

    def draws(self, sample_idx, seed=None, epoch: int = 0):
        """The decisions `batch(sample_idx, seed=seed, epoch=epoch)` takes from the Philox stream: offset (B,) int32,
        mirror (B, 2) bool, degrees (B,) int32 (-1: no rotation), noise_mask (B, obs, J - 1) bool and noise
        (B, obs, J - 1, 3) float32, already multiplied by noise_std.  The probabilities are applied; whether a
        batch uses mirror / degrees is its `train` flag's business."""
        self._require_device()
        idx = self._index(sample_idx)
        B, J, dev = idx.numel(), self.num_joints, self.device
        offset = torch.empty(B, device=dev, dtype=torch.int32)
        mirror = torch.empty(B, 2, device=dev, dtype=torch.uint8)
        degrees = torch.empty(B, device=dev, dtype=torch.int32)
        mask = torch.zeros(B, self.obs_length, J - 1, device=dev, dtype=torch.uint8)
        noise = torch.zeros(B, self.obs_length, J - 1, 3, device=dev, dtype=torch.float32)
        p = (lambda t: t.data_ptr()) if B else (lambda t: None)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(_lib.lib().sd_motion_draws(p(idx), B, J, self.obs_length, self.augmentation, self.da_mirroring, self.da_rotations,
                                         self.noise_level, self.noise_std, int(0 if seed is None else seed) & (2 ** 64 - 1),
                                         int(epoch), p(offset), p(mirror), p(degrees),
                                         p(mask) if self.if_noisy_obs else None, p(noise) if self.if_noisy_obs else None,
                                         stream))
        return {"offset": offset, "mirror": mirror.bool(), "degrees": degrees, "noise_mask": mask.bool(), "noise": noise}

    def batches(self, batch_size: int, *, train: bool, shuffle: bool, seed: int = 0, epoch: int = 0, drop_last: bool = False):
        """An epoch: yields batch(...) results over a device randperm of range(len(self)) (shuffle) or in order.
        The permutation is a function of (seed, epoch); nothing here reads the device back."""
        self._require_device()
        n = len(self)
        if shuffle:
            g = torch.Generator(device=self.device)
            g.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(epoch)) & (2 ** 63 - 1))
            order = torch.randperm(n, device=self.device, generator=g)
        else:
            order = torch.arange(n, device=self.device)
        for a in range(0, n, batch_size):
            if drop_last and a + batch_size > n:
                break
            yield self.batch(order[a:a + batch_size], train=train, seed=seed, epoch=epoch)

    # ---- every segment, unaugmented ----------------------------------------------------------------------------
    def _all_segments(self):
        self._require_device()
        idx = torch.arange(self.nseg, device=self.device)
        return self._launch(idx, False, 0, 0, None, 1, 0, False)

    def all_futures(self) -> torch.Tensor:
        """(nseg, pred_length, J_full - 1, 3): the future of every segment in input space, no offset, noise or
        augmentation: what MultimodalGT.mmade / mmfde / gt_apd take as `futures`."""
        return self._all_segments()[1]

    def last_obs(self) -> torch.Tensor:
        """(nseg, J_full - 1, 3): the last observed frame of every segment in input space (apply
        `representation.transform_to_metric_space` before multimodal_gt.get_multimodal_gt, as the reference does)."""
        return self._all_segments()[0][:, -1].contiguous()


__all__ = ["DeviceMotionData", "MotionRepresentation", "generate_segments", "segment_index", "rotation_table", "REPRESENTATIONS"]
