"""Multimodal ground truth on one MI355X: sd_cdist, get_multimodal_gt and MultimodalGT.gt_apd
against the torch-op expressions of the reference on the same GPU, synthetic data at the two released test
splits' sizes: H36M N = 5,168 (observed pose D = 48, future D = 4,800) and AMASS N = 12,727 (D = 63, 7,560).

    cdist              multimodal_gt.cdist(x, x)  vs  torch.cdist(x, x, compute_mode='donot_use_mm_for_euclid_dist')
    get_multimodal_gt  the whole search (row chunks of 2048, d < thr, nonzero, CSR)  vs  the same chunks with
                       torch.cdist and nonzero (math_utils.py:59-110 without its Python dict)
    gt_apd             one sd_cdist + sd_set_mean_distance  vs  the reference's apd (multimodal.py:15-35) per set

Protocol: every timed call is warmed up at its own shape, then timed as wall clock between two device
synchronisations; the two sides alternate inside one repeat loop.  Per line: median / min / max, and the spread
(max - min) of the torch side as the yardstick for a difference.  Also the achieved bytes/s of the short-D cdist
against its N^2 * 4 B of stores and the achieved VALU operations/s of the long-D cdist against 3 N^2 D (subtract,
multiply, add per pair and feature).  One JSON document on stdout and in --out.

Usage: python tools/bench_mmgt.py [--repeats 5] [--warmup 1] [--out profiles/mmgt/bench_mmgt.json] [--small]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from skeletondiffusion_amd import multimodal_gt  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default, cast=int):
    if name in ARGS:
        i = ARGS.index(name)
        v = cast(ARGS[i + 1])
        del ARGS[i:i + 2]
        return v
    return default


REPEATS, WARMUP = _opt("--repeats", 5), _opt("--warmup", 1)
OUT = _opt("--out", "", str)
# (name, N, joints, future frames); --small: a rehearsal of the script, not a measurement
SPLITS = [("h36m", 5168, 16, 100), ("amass", 12727, 21, 120)]
if "--small" in ARGS:
    SPLITS = [("small", 700, 16, 10)]
THR, CHUNK = 0.5, 2048
cuda = torch.device("cuda:0")
NO_MM = "donot_use_mm_for_euclid_dist"


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def versus(hip_fn, torch_fn, torch_repeats=None):
    """Both sides warmed up, then alternated; -> (hip stats, torch stats, last results)."""
    for _ in range(WARMUP):
        rh, rt = hip_fn(), torch_fn()
    torch.cuda.synchronize()
    h, t = [], []
    for i in range(REPEATS):
        ms, rh = sync_time(hip_fn)
        h.append(ms)
        if torch_repeats is None or i < torch_repeats:
            ms, rt = sync_time(torch_fn)
            t.append(ms)

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "all_ms": v}

    return stats(h), stats(t), rh, rt


def line(name, hip, tor, **extra):
    d = {"what": name, "hip": hip, "torch_ops": tor, "ratio_torch_over_hip": tor["median_ms"] / hip["median_ms"],
         "hip_not_slower_beyond_torch_spread": hip["median_ms"] <= tor["median_ms"] + tor["spread_ms"], **extra}
    print(json.dumps(d), flush=True)
    return d


def torch_mmgt(x):
    N = x.shape[0]
    rows, cols = [], []
    for r0 in range(0, N, CHUNK):
        hit = (torch.cdist(x[r0:r0 + CHUNK], x, p=2, compute_mode=NO_MM) < THR).nonzero()
        rows.append(hit[:, 0] + r0)
        cols.append(hit[:, 1])
    rows, col = torch.cat(rows), torch.cat(cols)
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=x.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return row_ptr, col


def torch_gt_apd(g, flat):
    """apd(mm_gt_i[None]) per segment (multimodal.py:15-35): cdist, the upper triangle, its mean."""
    rp = g.row_ptr_host.tolist()
    out = torch.zeros(len(g), device=flat.device)
    for i in range(len(g)):
        n = rp[i + 1] - rp[i]
        if n > 1:
            arr = flat[g.col[rp[i]:rp[i + 1]]][None]
            d = torch.cdist(arr, arr)
            iu = torch.triu_indices(n, n, offset=1)
            out[i] = d[:, iu[0], iu[1]].mean(dim=-1)[0]
    return out


results = []
for name, N, J, frames in SPLITS:
    g = torch.Generator().manual_seed(N)
    D0, D1 = 3 * J, 3 * J * frames
    members = 48  # segments per cluster; the jitter puts about half of a cluster's pairs inside the threshold
    centres = torch.randn((N + members - 1) // members, D0, generator=g) * 0.3
    obs = (centres[torch.arange(N) // members] + torch.randn(N, D0, generator=g) * (0.05 * (48 / D0) ** 0.5)).to(cuda)
    fut = torch.randn(N, D1, generator=g).to(cuda)
    shape = {"split": name, "N": N}

    for D, x in ((D0, obs), (D1, fut)):
        # the per-element torch kernel takes seconds at the long D: fewer repeats there
        hip, tor, dh, dt = versus(lambda: multimodal_gt.cdist(x, x), lambda: torch.cdist(x, x, p=2, compute_mode=NO_MM),
                                  torch_repeats=None if D == D0 else 3)
        sec = hip["median_ms"] * 1e-3
        extra = {"max_abs_hip_minus_torch": float((dh - dt).abs().max()),
                 "hip_bitwise_symmetric": bool(torch.equal(dh, dh.T)), "torch_bitwise_symmetric": bool(torch.equal(dt, dt.T))}
        if D == D0:
            extra["hip_store_TBps"] = N * N * 4 / sec / 1e12
        else:
            extra["hip_valu_Tops"] = 3.0 * N * N * D / sec / 1e12
        results.append(line("cdist", hip, tor, **shape, D=D, **extra))
        del dh, dt

    hip, tor, gh, (rp_t, col_t) = versus(lambda: multimodal_gt.get_multimodal_gt(obs, THR, CHUNK), lambda: torch_mmgt(obs))
    sizes = gh.row_ptr_host[1:] - gh.row_ptr_host[:-1]
    results.append(line("get_multimodal_gt", hip, tor, **shape, D=D0, hits=int(gh.col.numel()), max_set=int(sizes.max()),
                        mean_set=float(sizes.double().mean()), torch_hits=int(col_t.numel()),
                        same_hits_as_torch=bool(torch.equal(gh.col, col_t))))

    hip, tor, ah, at = versus(lambda: gh.gt_apd(fut), lambda: torch_gt_apd(gh, fut), torch_repeats=2)
    many = sizes.to(cuda) > 1
    results.append(line("gt_apd", hip, tor, **shape, D=D1,
                        max_rel_hip_minus_torch=float(((ah - at)[many].abs() / at[many]).max()) if bool(many.any()) else 0.0))
    del obs, fut, ah, at
    torch.cuda.empty_cache()

doc = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "warmup": WARMUP, "threshold": THR, "chunk_rows": CHUNK,
       "lines": results}
if OUT:
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
