"""Diversity ranking on one MI355X: metrics.diverse_rank (sd_diverse_rank: two launches) against
the torch-op expression on the same GPU: a batched torch.cdist of [target; pred] and the farthest-point greedy
restated with device ops, batched over the sequences (no Python loop per sequence, no host round trip: the
reference's own form, ranking.py:3-40, is a Python loop with .tolist() per pick and is not the comparator).

Shapes: 256 sequences x 50 samples, (frames, joints) = (100, 16) and (120, 21), n = 5; synthetic random walks
around the target.

Protocol: 3 warm-up calls per side, then `rounds` rounds in which the two sides alternate; a side's round is
`inner` back-to-back calls between two device events, `inner` sized so that a round takes about a quarter of a
second.  Per side: the median per-call time over the rounds and the spread (min, max).  Also the algorithmic
bytes nseq * (S + 1) * features * 4 over the HIP time, and its VALU operation rate against 3 * nseq * pairs *
features (subtract, multiply, add per pair and feature; pairs = (S + 1) S / 2, the upper triangle).
One JSON document on stdout and in --out.

Usage: python tools/bench_rank.py [--rounds 7] [--out profiles/rank/bench.json] [--small]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from skeletondiffusion_amd import metrics  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default, cast=int):
    if name in ARGS:
        i = ARGS.index(name)
        v = cast(ARGS[i + 1])
        del ARGS[i:i + 2]
        return v
    return default


ROUNDS, WARMUP, TARGET_S = _opt("--rounds", 7), 3, 0.25
OUT = _opt("--out", "", str)
NSEQ, SAMPLES, N_CHOOSE = 256, 50, 5
SHAPES = [(100, 16), (120, 21)]
if "--small" in ARGS:  # a rehearsal of the script, not a measurement
    NSEQ, SHAPES, TARGET_S = 8, [(10, 16)], 0.02
cuda = torch.device("cuda:0")


def torch_rank(pred, target, n):
    """batched torch.cdist + the greedy with device ops -> (idx (B, n), score (B, n))"""
    B, S = pred.shape[:2]
    arr = torch.cat([target.unsqueeze(1), pred], dim=1).reshape(B, S + 1, -1)
    dist = torch.cdist(arr, arr)
    m = dist[:, 0].clone()
    free = torch.ones(B, S + 1, dtype=torch.bool, device=pred.device)
    free[:, 0] = False
    rows = torch.arange(B, device=pred.device)
    idx, score = [], []
    for _ in range(n):
        val, c = torch.where(free, m, torch.full_like(m, -1.0)).max(dim=1)
        idx.append(c - 1)
        score.append(val)
        free[rows, c] = False
        m = torch.minimum(m, dist[rows, c])
    return torch.stack(idx, 1), torch.stack(score, 1)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, r


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "all_ms": v}


lines = []
for frames, joints in SHAPES:
    g = torch.Generator().manual_seed(frames * joints)
    tgt = torch.randn(NSEQ, frames, joints, 3, generator=g)
    steps = 0.03 * torch.randn(NSEQ, SAMPLES, frames, joints, 3, generator=g)
    pred = (tgt[:, None] + steps.cumsum(2) * (0.1 + 0.9 * torch.rand(NSEQ, SAMPLES, 1, 1, 1, generator=g))).to(cuda)
    tgt = tgt.to(cuda)
    sides = {"hip": lambda: metrics.diverse_rank(pred, tgt, N_CHOOSE), "torch_ops": lambda: torch_rank(pred, tgt, N_CHOOSE)}
    inner, res = {}, {}
    for name, fn in sides.items():
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ms, _ = timed(fn, 3)
        inner[name] = max(1, min(2000, int(TARGET_S * 1e3 / max(ms, 1e-3))))
    times = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            ms, res[name] = timed(fn, inner[name])
            times[name].append(ms)
    features = frames * joints * 3
    hip, tor = stats(times["hip"]), stats(times["torch_ops"])
    sec = hip["median_ms"] * 1e-3
    pairs = (SAMPLES + 1) * SAMPLES // 2
    d = {"what": "diverse_rank", "nseq": NSEQ, "samples": SAMPLES, "frames": frames, "joints": joints, "features": features,
         "n_choose": N_CHOOSE, "inner_calls": inner, "hip": hip, "torch_ops": tor,
         "ratio_torch_over_hip": tor["median_ms"] / hip["median_ms"],
         "same_picks_as_torch_ops": bool(torch.equal(res["hip"].idx, res["torch_ops"][0])),
         "algorithmic_bytes": NSEQ * (SAMPLES + 1) * features * 4,
         "hip_algorithmic_TBps": NSEQ * (SAMPLES + 1) * features * 4 / sec / 1e12,
         "hip_valu_Tops_upper_triangle": 3.0 * NSEQ * pairs * features / sec / 1e12}
    print(json.dumps(d), flush=True)
    lines.append(d)
    del pred, tgt, steps
    torch.cuda.empty_cache()

doc = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "warmup": WARMUP, "round_target_s": TARGET_S, "lines": lines}
if OUT:
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
