"""Shared by tests/test_motion_batch_host.py, tests/test_gpu_motion_batch.py and tools/bench_data.py: the cases of
tests/golden/motion_batch.npz and a torch-op restatement of sd_motion_batch.

The restatement takes one f32 operation at a time in the kernel's order (x + noise; the sign; c x - s y and
s x + c y as two products and a difference / sum; x - hip; a division by a tensor), so on a backend with IEEE f32
arithmetic -- the CPU, where the tests run it -- it rounds exactly as the kernel does."""
import numpy as np
import torch

from conftest import golden

# case -> (settings of DeviceMotionData, train flag)
TRAIN = dict(stride=3, augmentation=2, da_mirroring=0.5, da_rotations=0.5)
CASES = {
    "train_j17": (dict(TRAIN, motion_repr_type="SkeletonRescalePose", pose_box_size=1.5), True),
    "train_j22": (dict(TRAIN, motion_repr_type="SkeletonRescalePose", pose_box_size=1.5), True),
    "train_j52": (dict(TRAIN, motion_repr_type="SkeletonRescalePose", pose_box_size=1.5), True),
    "train_center_j17": (dict(TRAIN, motion_repr_type="SkeletonCenterPose"), True),
    "noisy_j17": (dict(if_noisy_obs=True, noise_level=0.3, noise_std=0.03, motion_repr_type="SkeletonRescalePose",
                       pose_box_size=1.5), False),
    "segments_j17": (dict(motion_repr_type="SkeletonRescalePose", pose_box_size=1.5), False),
}
TRAIN_CASES = [c for c, (_, train) in CASES.items() if train]
DRAW_KEYS = ("offset", "mirror", "degrees", "noise_mask", "noise")

_z = None


def fixture():
    global _z
    if _z is None:
        _z = golden("motion_batch")
    return _z


def case_arrays(case):
    z = fixture()
    return {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}


def case_clips(a):
    """The case's clips as a list of (T_i, J, 3) arrays."""
    return np.split(a["clips"], np.cumsum(a["clip_lengths"])[:-1])


def case_data(case, device, **override):
    """DeviceMotionData of a fixture case (its explicit segment list for segments_j17)."""
    from skeletondiffusion_amd.data import DeviceMotionData

    a = case_arrays(case)
    z = fixture()
    kw = dict(CASES[case][0], **override)
    if case == "segments_j17":
        kw["segments"] = a["segments"][:, :2]
    return DeviceMotionData(case_clips(a), int(z["obs_length"]), int(z["pred_length"]), device=device, **kw), a


def case_draws(a):
    return {k: a[k] for k in DRAW_KEYS}


def raw_max(a):
    """M of the derived bounds: the largest raw |coordinate| of the case."""
    return float(np.abs(a["clips"]).max())


def restate(frames, seg_first, sample_idx, obs_len, pred_len, *, stride=1, augmentation=0, train=False, noisy=False,
            representation="SkeletonRescalePose", pose_box_size=1.5, draws=None, rot_table=None):
    """sd_motion_batch in torch ops on frames' device: obs, pred, segment_idx.  frames (F, J, 3) f32, seg_first
    (nseg,) int64, sample_idx (B,) int64, draws as DeviceMotionData.draws returns them, rot_table (720,) f32."""
    dev = frames.device
    t = lambda v, dt: torch.as_tensor(v).to(device=dev, dtype=dt)
    nseg = seg_first.numel()
    seg = stride * sample_idx + augmentation
    if augmentation != 0:
        seg = seg + t(draws["offset"], torch.int64)
    seg = seg.clamp(0, nseg - 1)
    steps = torch.arange(obs_len + pred_len, device=dev)
    x = frames[seg_first[seg][:, None] + steps[None]]  # (B, seg, J, 3), a copy
    if noisy:
        mask, noise = t(draws["noise_mask"], torch.bool), t(draws["noise"], torch.float32)
        part = x[:, :obs_len, 1:]
        x[:, :obs_len, 1:] = torch.where(mask[..., None], part + noise, part)
    if train:
        mirror = t(draws["mirror"], torch.bool)
        for m in (0, 1):
            x[..., m] = torch.where(mirror[:, m, None, None], -x[..., m], x[..., m])
        deg = t(draws["degrees"], torch.int64)
        d = deg.clamp(min=0) % 360
        c, s = rot_table[d][:, None, None], rot_table[360 + d][:, None, None]
        x0, x1 = x[..., 0].clone(), x[..., 1].clone()
        rot = (deg >= 0)[:, None, None]
        x[..., 0] = torch.where(rot, c * x0 - s * x1, x0)
        x[..., 1] = torch.where(rot, s * x0 + c * x1, x1)
    if representation != "SkeletonVanilla":
        x = x - x[..., 0:1, :]
        if representation == "SkeletonRescalePose":
            x = x / torch.tensor(pose_box_size, dtype=torch.float32, device=dev)
    x = x[..., 1:, :]
    return x[:, :obs_len].contiguous(), x[:, obs_len:].contiguous(), seg


def restate_data(data, sample_idx, *, train, draws, device="cpu"):
    """`restate` with the settings and tables of a DeviceMotionData, computed on `device`."""
    dev = torch.device(device)
    idx = torch.as_tensor(sample_idx).to(device=dev, dtype=torch.int64).reshape(-1)
    d = None if draws is None else {k: torch.as_tensor(v).to(dev) for k, v in draws.items()}
    return restate(data.frames.to(dev), data.seg_first.to(dev), idx, data.obs_length, data.pred_length, stride=data.stride,
                   augmentation=data.augmentation, train=train, noisy=data.if_noisy_obs, representation=data.motion_repr_type,
                   pose_box_size=data.pose_box_size, draws=d, rot_table=data.rot_table.to(dev))


def bits_equal(a, b):
    """Bitwise equality of two float32 tensors / arrays (-0.0 and 0.0 differ, NaN payloads count)."""
    a, b = (np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32) for v in (a, b))
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def synthetic_clips(lengths, J, seed):
    """Clips with a wandering hip and |coordinate| up to ~3, as the fixture's."""
    rs = np.random.RandomState(seed)
    out = []
    for T in lengths:
        hip = np.cumsum(rs.randn(T, 1, 3) * 0.05, 0) + rs.uniform(-2, 2, (1, 1, 3))
        pose = rs.uniform(-0.9, 0.9, (1, J, 3))
        out.append((hip + pose + rs.randn(T, J, 3) * 0.02).astype(np.float32))
    return out
