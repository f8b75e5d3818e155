"""The optimizer tail of a training step alone: gradient-norm clipping + Adam / AdamW
over the four parameter sets of the two training loops, with synthetic gradients, as
  (a) torch:        clip_grad_norm_ + torch.optim.Adam / AdamW with their defaults,
  (b) torch_fused:  the same with fused=True, where this torch build accepts it,
  (c) hip:          optim.FusedAdam(max_grad_norm=1),
and, for the stage-2 sets, the EMA update alone: optim.EMA's launch against a per-parameter lerp_ loop.
One process; device-event timing of windows of --calls calls after a warm-up window; the variants
alternate and every variant gets --repeats windows, so the spread (min .. max of the windows) is known
before a difference is read.  Per variant: median and spread, the algorithmic bytes (from the element
counts, below), bytes/s, the share of the HBM peak, and the device kernels one call launches.
Writes profiles/optim/bench.json and prints it.
Usage: python tools/bench_optimizer.py [--sets d16,d21,d51,ae16] [--calls 200] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from conftest import build_release_diffusion, golden  # noqa: E402
from skeletondiffusion_amd import optim  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, the MI355X HBM3E specification (6.29e12 measured with a float4 copy)
DENOISER = {16: "release_h36m16_T10", 21: "release_amass21_T10", 51: "release_mano51_T10"}


def parameter_set(name, dev):
    """(module, stage): the release Denoiser (stage 2: Adam) or the autoencoder (stage 1: AdamW amsgrad)."""
    if name.startswith("d"):
        return build_release_diffusion(golden(DENOISER[int(name[1:])]), device=dev).model.train(), 2
    from bench_train_autoencoder import model
    return model(int(name[2:]), dev), 1


def algorithmic_bytes(numel, stage):
    """f32 arrays of `numel` elements moved per call: the norm reads g; the step reads p, g, m, v and
    writes p, m, v and the clipped g; amsgrad (stage 1) also reads and writes vmax."""
    return 4 * numel * (1 + 4 + 3 + 1 + (2 if stage == 1 else 0))


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def kernels_per_call(fn):
    """Device kernels one call launches, counted by the profiler (None where it is unavailable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA) or None
    except Exception:
        return None


def measure(variants, calls, repeats):
    for fn in variants.values():  # warm-up: one window each (allocations, lazy state)
        window_ms(fn, calls)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():  # alternate
            times[k].append(window_ms(fn, calls))
    return times


def summarise(ts, nbytes):
    med = statistics.median(ts)
    return {"median_us": med * 1e3, "min_us": min(ts) * 1e3, "max_us": max(ts) * 1e3, "windows_us": [t * 1e3 for t in ts],
            "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-3), "share_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK}


def bench_set(name, dev, calls, repeats):
    module, stage = parameter_set(name, dev)
    ps = [p for p in module.parameters() if p.requires_grad]
    numel = sum(p.numel() for p in ps)
    g = torch.Generator(device=dev).manual_seed(7)
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
    kw = dict(lr=1e-4, amsgrad=True, weight_decay=1e-2) if stage == 1 else dict(lr=1e-4)
    cls = torch.optim.AdamW if stage == 1 else torch.optim.Adam
    opts = {"torch": cls(ps, **kw)}
    try:
        o = cls(ps, fused=True, **kw)
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        o.step()
        torch.cuda.synchronize()
        opts["torch_fused"] = o
    except Exception as e:  # this build refuses fused=True here
        fused_note = f"{type(e).__name__}: {e}"
    else:
        fused_note = "accepted"
    hip = optim.FusedAdam(ps, decoupled_weight_decay=stage == 1, max_grad_norm=1.0, **kw)

    def torch_step(o):
        def fn():
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            o.step()
        return fn

    variants = {k: torch_step(o) for k, o in opts.items()}
    variants["hip"] = hip.step
    times = measure(variants, calls, repeats)
    nbytes = algorithmic_bytes(numel, stage)
    res = {"set": name, "stage": stage, "tensors": len(ps), "elements": numel, "torch_fused": fused_note,
           "optimizer": {k: dict(summarise(ts, nbytes), kernels_per_call=kernels_per_call(variants[k]))
                         for k, ts in times.items()}}
    a, c = res["optimizer"]["torch"], res["optimizer"]["hip"]
    res["hip_faster_than_torch_by_more_than_the_spread"] = c["max_us"] < a["min_us"]
    if stage == 2:
        ema = optim.EMA(module, update_every=1, update_after_step=0)
        pairs = ema._pairs()
        avg = [a for a, _ in pairs[1]]

        def lerp_loop():
            for a, p in zip(avg, ps):
                a.lerp_(p.detach(), 0.005)

        ev = {"lerp_loop": lerp_loop, "hip": lambda: ema._blend(pairs, 0.005)}
        et = measure(ev, calls, repeats)
        res["ema"] = {k: dict(summarise(ts, 4 * numel * 3), kernels_per_call=kernels_per_call(ev[k])) for k, ts in et.items()}
    for p in ps:
        p.grad = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="d16,d21,d51,ae16")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim", "bench.json"))
    a = ap.parse_args()
    assert a.calls >= 200 and a.repeats >= 5
    dev = torch.device("cuda:0")
    rows = []
    for name in a.sets.split(","):
        rows.append(bench_set(name, dev, a.calls, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    res = {"metric": "optimizer tail of a training step, microseconds per call (gradient-norm clip + Adam / AdamW; EMA update)",
           "device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "windows": a.repeats,
           "hbm_peak_bytes_per_s": HBM_PEAK, "infinity_cache_hits_of_the_second_gradient_read": "not measured",
           "sets": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "sets"}))


if __name__ == "__main__":
    main()
