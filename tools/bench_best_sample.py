"""Time the best-sample selection (sd_best_sample: per-sample distances, index, distance, best
trajectory and its tail) on one MI355X, or -- in a process of its own -- the torch-op expression a
user would write without it and a streaming copy of the same tensor as the bandwidth yardstick.
One implementation per process; prints one JSON line.

Usage: python tools/bench_best_sample.py hip|torch [sequences] [samples] [frames] [joints] [tail]"""
import json
import sys

import torch

sys.path.insert(0, ".")
from skeletondiffusion_amd import metrics  # noqa: E402

IMPL = sys.argv[1]
NSEQ, S, T, J, TAIL = (int(a) for a in (sys.argv[2:7] + ["256", "50", "120", "21", "30"][len(sys.argv) - 2:]))
WARM, ITERS = 3, 20
cuda = torch.device("cuda:0")
g = torch.Generator(device=cuda).manual_seed(3)
y = torch.randn(NSEQ, T, J, 3, device=cuda, generator=g) * 0.3
out = y.unsqueeze(1) + 0.1 * torch.randn(NSEQ, S, T, J, 3, device=cuda, generator=g)


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


def torch_expression():
    d = torch.linalg.norm(out - y.unsqueeze(1), dim=-1).mean(-1).mean(-1).min(-1)
    best = out[torch.arange(NSEQ, device=cuda), d.indices]
    return d.indices, d.values, best, best[:, T - TAIL:].contiguous()


L = T * J * 3
# what the algorithm has to move: pred and target once, the selected sample and its tail read and written
need = 4 * (NSEQ * S * L + NSEQ * L + 2 * NSEQ * (L + TAIL * J * 3) + 2 * NSEQ * S)
res = {"impl": IMPL, "shape": [NSEQ, S, T, J, 3], "tail": TAIL, "pred_MB": 4e-6 * NSEQ * S * L, "needed_MB": need * 1e-6}
if IMPL == "hip":
    r = timed(lambda: metrics.best_sample(out, y, tail=TAIL))
    res.update(r, GBps=need / r["median_ms"] * 1e-6)
    idx, dist, _, _ = metrics.best_sample(out, y, tail=TAIL)
    res.update(idx_head=idx[:4].tolist(), dist_mean=float(dist.mean()))
elif IMPL == "torch":
    r = timed(torch_expression)
    res.update(r, GBps_of_needed=need / r["median_ms"] * 1e-6)
    idx, dist, _, _ = torch_expression()
    res.update(idx_head=idx[:4].tolist(), dist_mean=float(dist.mean()))
    dst = torch.empty_like(out)
    c = timed(lambda: dst.copy_(out))
    res["stream_copy"] = dict(c, GBps=2 * 4 * out.numel() / c["median_ms"] * 1e-6)
else:
    raise SystemExit("first argument: hip or torch")
print(json.dumps(res))
