"""Time the fused body-realism / limb-angle / motion-profile call (metrics.realism: sd_realism_target +
sd_realism) on one MI355X with and without the angles, next to a streaming copy of the
same tensor (`dst.copy_(pred)`) as the bandwidth yardstick in the same process.  3 warm-up + 20 timed
calls, device events, median; prints one JSON line per shape.

With --torch the process runs ONLY the torch-op expression a user would write without this library (the
reference's functions in float32, dot products as (a * b).sum(-1)) and imports nothing of this package:
the limb tables come from tests/golden/realism.npz.  One implementation per process.

Usage: python tools/bench_realism.py [--torch] [sequences ...]     (default: 8 256; x 50 x 120 x 21 x 3)"""
import json
import math
import os
import sys

import numpy as np
import torch

ARGS = [a for a in sys.argv[1:] if a != "--torch"]
TORCH = "--torch" in sys.argv[1:]
SEQS = [int(a) for a in ARGS] or [8, 256]
S, T, J = 50, 120, 21
WARM, ITERS = 3, 20
cuda = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))


def timed(fn):
    for _ in range(WARM):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(ITERS + 1)]
    ev[0].record()
    for i in range(ITERS):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in zip(ev, ev[1:]))
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def inputs(nseq):
    g = torch.Generator(device=cuda).manual_seed(3)
    y = torch.randn(nseq, T, J, 3, device=cuda, generator=g) * 0.3
    return y.unsqueeze(1) + 0.1 * torch.randn(nseq, S, T, J, 3, device=cuda, generator=g), y


def torch_expression(pred, target, limbseq, pairs):
    """body_realism.py:109-199, multimodal.py:76-102 and cmd.py:10-12 in torch ops (float32)."""
    ll = (pred[..., limbseq[:, 0], :] - pred[..., limbseq[:, 1], :]).norm(dim=-1)  # (B, S, T, L)
    gt = (target[..., limbseq[:, 0], :] - target[..., limbseq[:, 1], :]).norm(dim=-1).mean(-2)[:, None]  # (B, 1, L)
    dev2 = ((ll - gt[:, :, None]) ** 2).mean(-2)
    jit = (ll[:, :, 1:] - ll[:, :, :-1]).abs()
    jit2 = (jit ** 2).mean(-2)
    out = [dev2.sqrt() / gt, dev2 / gt, jit2.sqrt() / gt, jit2 / gt, (ll.mean(-2) - gt).abs() / gt, jit.mean(-2) / gt]
    out = [v.flatten(1).mean(-1) for v in out]
    ls = limbseq.sort(dim=-1)[0]

    def cos(x):
        v = x[..., ls[:, 1], :] - x[..., ls[:, 0], :]
        a, b = v[..., pairs[:, 0], :], v[..., pairs[:, 1], :]
        return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-7)

    cp, cg = cos(pred), cos(target)[:, None]
    ang = (torch.acos(cp.clamp(-1, 1)) - torch.acos(cg.clamp(-1, 1))).abs().mean(-1).mean(-1) * (180 / math.pi)
    cs = (cp - cg).abs().mean(-1).mean(-1) * (180 / math.pi)
    motion = (pred[:, :, 1:] - pred[:, :, :-1]).norm(dim=-1).mean(1).mean(-1)
    return out, ang.min(-1).values, cs.min(-1).values, motion


for nseq in SEQS:
    pred, target = inputs(nseq)
    res = {"impl": "torch" if TORCH else "hip", "shape": [nseq, S, T, J, 3], "pred_MB": 4e-6 * pred.numel()}
    if TORCH:
        z = np.load(os.path.join(HERE, "..", "tests", "golden", "realism.npz"))
        limbseq = torch.from_numpy(z["amass21_limbseq"]).long().to(cuda)
        pairs = torch.from_numpy(z["amass21_angle_pairs"]).long().to(cuda)
        res["torch_ops"] = timed(lambda: torch_expression(pred, target, limbseq, pairs))
        out, ang, _, motion = torch_expression(pred, target, limbseq, pairs)
        res.update(smean_mean=float(out[4].mean()), mae_mean=float(ang.mean()), motion_mean=float(motion.mean()))
    else:
        sys.path.insert(0, os.path.join(HERE, ".."))
        from skeletondiffusion_amd import metrics, skeletons  # noqa: E402

        limbseq, chains = skeletons.limbseq("amass21"), skeletons.limb_angles_idx("amass21")
        res["fused_with_angles"] = timed(lambda: metrics.realism(pred, target, limbseq, chains))
        res["fused_without_angles"] = timed(lambda: metrics.realism(pred, target, limbseq))
        dst = torch.empty_like(pred)
        res["stream_copy"] = timed(lambda: dst.copy_(pred))
        res["stream_copy"]["GBps"] = 2 * 4 * pred.numel() / res["stream_copy"]["median_ms"] * 1e-6
        for k in ("fused_with_angles", "fused_without_angles"):
            res[k]["GBps_of_pred"] = 4 * pred.numel() / res[k]["median_ms"] * 1e-6
            res[k]["x_copy"] = res[k]["median_ms"] / res["stream_copy"]["median_ms"]
        r = metrics.realism(pred, target, limbseq, chains)
        res.update(smean_mean=float(r.smean_mean.mean()), mae_mean=float(r.mae.mean()), motion_mean=float(r.motion.mean()))
        del dst
    print(json.dumps(res), flush=True)
    del pred, target
