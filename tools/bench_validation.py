"""Time the validation metrics of a training loop's validation batch on one MI355X, two paths
in the same process on the same tensors, alternating call by call:

    hip     metrics.limb_stats(pred, limbseq, target) + MPJPEAccumulator.update(best=True) + FDEAccumulator.update(idx)
            (sd_limb_stats, sd_best_sample, sd_frame_error_update)
    torch   the same quantities written with torch ops on the device tensors, the reference's formulas in float32
            (body_realism.py:4-107, metrics/utils.py:12-20, ignite_mpjpe.py, ignite_fde.py), the sums kept on the device

and, each on its own, the limb-statistics call, the two accumulator updates, and a streaming copy of pred
(`dst.copy_(pred)`) as the bandwidth yardstick.  3 warm-up calls of everything, then 21 timed rounds; device events;
median, minimum and maximum per entry (the spread of the run).  Prints one JSON line per shape and, with --out DIR,
writes them to DIR/bench.json.

Usage: python tools/bench_validation.py [--out DIR] [--small]     (--small: 4 sequences, a rehearsal of the code path)"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from skeletondiffusion_amd import metrics, skeletons  # noqa: E402

SMALL = "--small" in sys.argv[1:]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else None
NSEQ = 4 if SMALL else 256
SHAPES = [(NSEQ, 50, 100, 16, "h36m16"), (NSEQ, 50, 120, 21, "amass21")]
WARM, ROUNDS = 3, 21
cuda = torch.device("cuda:0")


def inputs(B, S, T, J):
    g = torch.Generator(device=cuda).manual_seed(5)
    y = torch.randn(B, T, J, 3, device=cuda, generator=g) * 0.3
    return y.unsqueeze(1) + 0.1 * torch.randn(B, S, T, J, 3, device=cuda, generator=g), y


def torch_limb_stats(pred, target, ls):
    """body_realism.py:4-107 in torch ops (float32): every quantity `LimbStats` holds."""
    ll = (pred[..., ls[:, 0], :] - pred[..., ls[:, 1], :]).norm(dim=-1)      # (B, S, T, L)
    tl = (target[..., ls[:, 0], :] - target[..., ls[:, 1], :]).norm(dim=-1)  # (B, T, L)
    var = ll.var(dim=-2)
    jit = (ll[..., 1:, :] - ll[..., :-1, :]).abs()
    err = (tl.unsqueeze(1) - ll).abs().mean(-2)
    out = [var, jit, err]
    for v, red in ((var, None), (jit, -2)):
        per_limb = (v,) * 3 if red is None else (v.mean(red), v.max(red).values, v.min(red).values)
        ps = (per_limb[0].mean(-1), per_limb[1].max(-1).values, per_limb[2].min(-1).values)
        out += [*per_limb, *ps, ps[0].mean(-1), ps[1].max(-1).values, ps[2].min(-1).values]
    eps = err.mean(-1)
    return out + [eps, eps.mean(-1), eps.max(-1).values, eps.min(-1).values]


class TorchFrameError:
    """The per-frame MPJPE and FDE sums of the best sample with torch ops; the state stays on the device."""

    def __init__(self):
        self.sum, self.count = None, 0

    def update(self, pred, target):
        idx = (pred - target.unsqueeze(1)).norm(dim=-1).mean(-1).mean(-1).min(dim=-1).indices  # metrics/utils.py:14
        best = pred[torch.arange(pred.shape[0], device=pred.device), idx]                    # the gathered copy
        e = (best - target).norm(dim=-1).to(torch.float64).sum(0)                            # (T, J)
        self.sum = e if self.sum is None else self.sum + e
        self.count += pred.shape[0]


def measure(entries):
    """entries: name -> callable.  Warm everything, then ROUNDS rounds calling each entry once, in turn."""
    for _ in range(WARM):
        for fn in entries.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in entries}
    for _ in range(ROUNDS):
        for k, fn in entries.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            times[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, evs in times.items():
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        out[k] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}
    return out


lines = []
for B, S, T, J, skel in SHAPES:
    pred, target = inputs(B, S, T, J)
    limbseq = skeletons.limbseq(skel)
    ls = torch.tensor(limbseq, device=cuda)
    dst = torch.empty_like(pred)
    mp, fd, tf = metrics.MPJPEAccumulator(device=cuda), metrics.FDEAccumulator(device=cuda), TorchFrameError()

    def hip_updates():
        idx = metrics.best_sample(pred, target)[0]
        mp.update(pred, target, idx=idx)
        fd.update(pred, target, idx=idx)

    def hip_all():
        metrics.limb_stats(pred, limbseq, target)
        hip_updates()

    def torch_all():
        torch_limb_stats(pred, target, ls)
        tf.update(pred, target)

    res = {"shape": [B, S, T, J, 3], "pred_MB": 4e-6 * pred.numel(), "warmup": WARM}
    res.update(measure({"hip": hip_all, "torch": torch_all,
                        "hip_limb_stats": lambda: metrics.limb_stats(pred, limbseq, target),
                        "torch_limb_stats": lambda: torch_limb_stats(pred, target, ls),
                        "hip_accumulators": hip_updates, "torch_accumulators": lambda: tf.update(pred, target),
                        "hip_limb_variance_only": lambda: metrics.limb_length_variance(pred, limbseq),
                        "stream_copy": lambda: dst.copy_(pred)}))
    res["stream_copy"]["GBps"] = 2 * 4 * pred.numel() / res["stream_copy"]["median_ms"] * 1e-6
    for k in ("hip_limb_stats", "hip_limb_variance_only"):
        res[k]["GBps_of_pred"] = 4 * pred.numel() / res[k]["median_ms"] * 1e-6
        res[k]["x_copy"] = res[k]["median_ms"] / res["stream_copy"]["median_ms"]
    res["torch_over_hip"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    # the two paths computed the same thing (float32 torch against float64 kernels: loose)
    r, t = metrics.limb_stats(pred, limbseq, target), torch_limb_stats(pred, target, ls)
    res["check"] = {"variance_mean": [float(r.variance_mean.mean()), float(t[9].mean())],
                    "jitter_max": [float(r.jitter_max.max()), float(t[19].max())],
                    "error_mean": [float(r.error_mean.mean()), float(t[22].mean())],
                    "mpjpe_sum": [float(mp.sum.sum() / int(mp.count)), float(tf.sum.sum() / tf.count)]}
    print(json.dumps(res), flush=True)
    lines.append(res)
    del pred, target, dst
if OUT:
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "bench.json"), "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
