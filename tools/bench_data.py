"""Motion batches on one MI355X: how fast a training batch is built.

Workload: a synthetic clip set of 150 clips x 3,000 frames, obs 25, pred 100, J_full = 17 and 22, the release
augmentation settings (stride 10, augmentation 5, mirroring 0.5, rotations 1.0, SkeletonRescalePose box 1.5), batches
of B = 64 and 1,024 random samples.  Three ways to the same batch, in one process, alternating, after warm-up:

    (a) hip         DeviceMotionData.batch: one kernel over the resident clips
    (b) torch_ops   the torch-op restatement (tests/motion_batch_cases.py:restate) on the same GPU, same draws
    (c) host_loader a host restatement of the reference's per-item path (numpy slice, np.random draws, sign flips,
                    the rotation matrix from scipy if importable, torch centring / division / root drop; no
                    observation noise, which the release configs leave off), default_collate and the
                    host-to-device copy, single process -- what one DataLoader worker does for a batch

Every call is timed on its own, wall clock between two device synchronisations; per line the median, min, max and
spread, and samples/s from the median.  For (a) also the kernel's algorithmic bytes (read B seg J 12, written
B seg (J - 1) 12) over its time, as a share of the 8.0 TB/s HBM peak: a call's time includes the launch and the
output allocations, so this is a lower bound of the kernel's own share.  `workers_to_feed` is how many host
workers of rate (c) a consumer needs: stage 2 at 116k samples/s, stage 1 at 64 rows per 3.2 - 15.7 ms.
The one condition: (a) is not slower than (b).  A run that finds no GPU fails.

Usage: python tools/bench_data.py [--repeats 30] [--warmup 5] [--out profiles/data/bench.json] [--small]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.utils.data._utils.collate import default_collate

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from skeletondiffusion_amd.data import DeviceMotionData, rotation_table  # noqa: E402
import motion_batch_cases as C  # noqa: E402

try:
    from scipy.spatial.transform import Rotation as R
except ImportError:  # the rotation matrix from the table instead
    R = None

ARGS = sys.argv[1:]


def _opt(name, default, cast=int):
    if name in ARGS:
        i = ARGS.index(name)
        v = cast(ARGS[i + 1])
        del ARGS[i:i + 2]
        return v
    return default


REPEATS, WARMUP = _opt("--repeats", 30), _opt("--warmup", 5)
OUT = _opt("--out", "", str)
CLIPS, FRAMES, OBS, PRED = 150, 3000, 25, 100
if "--small" in ARGS:  # a rehearsal of the script, not a measurement
    CLIPS, FRAMES = 6, 400
SETTINGS = dict(stride=10, augmentation=5, da_mirroring=0.5, da_rotations=1.0, motion_repr_type="SkeletonRescalePose",
                pose_box_size=1.5)
HBM_PEAK = 8.0e12
CONSUMERS = {"stage2_116k_samples_per_s": 116e3, "stage1_fast_64_rows_per_3.2ms": 64 / 3.2e-3,
             "stage1_slow_64_rows_per_15.7ms": 64 / 15.7e-3}

if not torch.cuda.is_available():
    sys.exit("bench_data: no GPU found; this is a measurement and has no fallback")
cuda = torch.device("cuda:0")


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(v, B):
    med = statistics.median(v)
    return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "samples_per_s": B / (med * 1e-3)}


def host_loader(clips, segments, sample_idx, rot_tab):
    """The reference's per-item path restated (base_dataset.py:109-133, motion_dataset.py:129-193), one item at a
    time, then default_collate and the copy to the device."""
    seg_len, items = OBS + PRED, []
    for s in sample_idx:
        k = int(SETTINGS["stride"] * s + SETTINGS["augmentation"])
        k = max(0, min(k + np.random.randint(-SETTINGS["augmentation"], SETTINGS["augmentation"] + 1), len(segments) - 1))
        ci, init = segments[k]
        data = clips[ci][init:init + seg_len]
        obs, pred = data[:OBS], data[OBS:]
        for m in (0, 1):
            if np.random.rand() < SETTINGS["da_mirroring"]:
                obs, pred = obs.copy(), pred.copy()
                obs[..., m] *= -1
                pred[..., m] *= -1
        if np.random.rand() < SETTINGS["da_rotations"]:
            deg = np.random.randint(0, 360)
            if R is not None:
                r = R.from_euler("z", deg, degrees=True).as_matrix().astype(np.float32)
            else:
                c, sn = rot_tab[deg], rot_tab[360 + deg]
                r = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]], np.float32)
            obs = (r @ obs.reshape((-1, 3)).T).T.reshape(obs.shape)
            pred = (r @ pred.reshape((-1, 3)).T).T.reshape(pred.shape)
        x = torch.cat([torch.from_numpy(obs), torch.from_numpy(pred)], dim=-3)
        x = (x - x[..., 0:1, :]) / SETTINGS["pose_box_size"]
        x = x[..., 1:, :]
        items.append((x[:OBS], x[OBS:], {"sample_idx": int(s), "clip_idx": int(ci), "init": int(init), "end": int(init + seg_len - 1),
                                         "segment_idx": k}))
    obs, pred, extra = default_collate(items)
    return obs.to(cuda), pred.to(cuda), {k: v.to(cuda) for k, v in extra.items()}


lines = []
for J in (17, 22):
    rs = np.random.RandomState(J)
    clips = [(np.cumsum(rs.randn(FRAMES, 1, 3).astype(np.float32) * 0.05, 0) + rs.uniform(-0.9, 0.9, (1, J, 3)).astype(np.float32) +
              rs.randn(FRAMES, J, 3).astype(np.float32) * 0.02).astype(np.float32) for _ in range(CLIPS)]
    data = DeviceMotionData(clips, OBS, PRED, device=cuda, **SETTINGS)
    segments = data.segments.tolist()
    rot_tab = rotation_table()
    for B in (64, 1024):
        idx = torch.from_numpy(np.random.RandomState(B).permutation(len(data))[:B].astype(np.int64)).to(cuda)
        idx_host = idx.cpu().tolist()
        draws = data.draws(idx, 1, 0)

        def hip():
            return data.batch(idx, train=True, seed=1, epoch=0)

        def torch_ops():
            return C.restate(data.frames, data.seg_first, idx, OBS, PRED, stride=data.stride, augmentation=data.augmentation,
                             train=True, noisy=False, representation=data.motion_repr_type, pose_box_size=data.pose_box_size,
                             draws=draws, rot_table=data.rot_table)

        def host():
            return host_loader(clips, segments, idx_host, rot_tab)

        host_repeats = max(3, REPEATS // 10) if B > 64 else max(5, REPEATS // 3)
        for _ in range(WARMUP):
            a, b = hip(), torch_ops()
        host()
        t = {"hip": [], "torch_ops": [], "host_loader": []}
        for i in range(REPEATS):
            ms, a = sync_time(hip)
            t["hip"].append(ms)
            ms, b = sync_time(torch_ops)
            t["torch_ops"].append(ms)
            if i < host_repeats:
                ms, _ = sync_time(host)
                t["host_loader"].append(ms)
        err = max(float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()))
        st = {k: stats(v, B) for k, v in t.items()}
        bytes_moved = B * (OBS + PRED) * (J + J - 1) * 12
        line = {"J_full": J, "B": B, "obs": OBS, "pred": PRED, "frames_resident": data.total_frames, "samples_per_epoch": len(data),
                **st, "ratio_torch_over_hip": st["torch_ops"]["median_ms"] / st["hip"]["median_ms"],
                "hip_not_slower_than_torch_ops": st["hip"]["median_ms"] <= st["torch_ops"]["median_ms"],
                "max_abs_hip_minus_torch_ops": err, "hip_algorithmic_bytes": bytes_moved,
                "hip_call_share_of_hbm_peak": bytes_moved / (st["hip"]["median_ms"] * 1e-3) / HBM_PEAK,
                "host_rotation": "scipy" if R is not None else "table",
                "workers_to_feed": {k: rate / st["host_loader"]["samples_per_s"] for k, rate in CONSUMERS.items()}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    del data
    torch.cuda.empty_cache()

doc = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "warmup": WARMUP, "clips": CLIPS, "frames_per_clip": FRAMES,
       "settings": SETTINGS, "hbm_peak_bytes_per_s": HBM_PEAK, "consumers_samples_per_s": CONSUMERS, "lines": lines,
       "hip_not_slower_than_torch_ops_everywhere": all(l["hip_not_slower_than_torch_ops"] for l in lines)}
if OUT:
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
