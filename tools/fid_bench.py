"""FID accumulation of one evaluation batch on one MI355X: the HIP path
(metrics.FIDAccumulator.update: sd_fid_features on pred and target, sd_fid_stats_update twice) against the
torch-op expression of the reference's storer on the same GPU (src/metrics/fid.py:106-123: reshape,
permute(0, 2, 1), permute(2, 0, 1).contiguous(), nn.GRU(48, 128, 2), tanh(linear1(.)), and the activations
copied to the host after every batch), same synthetic weights, same inputs.

Both sides are timed as wall-clock per batch with the device idle before and after (the torch-op side ends in
its own host copy; the HIP side is followed by a synchronize, which the pipeline does not need).  One JSON
line: median / min / max over the repeats, the ratio, the largest feature difference between the two paths and
the HIP features' largest error against a float64 run of the first rows on the CPU.

Usage: python tools/fid_bench.py [sequences=256] [samples=50] [frames=100] [--repeats 7] [--warmup 2]"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from skeletondiffusion_amd import metrics, synthetic  # noqa: E402

ARGS = sys.argv[1:]


def _opt(name, default):
    if name in ARGS:
        i = ARGS.index(name)
        v = int(ARGS[i + 1])
        del ARGS[i:i + 2]
        return v
    return default


REPEATS, WARMUP = _opt("--repeats", 7), _opt("--warmup", 2)
B = int(ARGS[0]) if len(ARGS) > 0 else 256
S = int(ARGS[1]) if len(ARGS) > 1 else 50
T = int(ARGS[2]) if len(ARGS) > 2 else 100
J, H, FEAT = 16, 128, 30
cuda = torch.device("cuda:0")

shapes = {"linear1.weight": (FEAT, H), "linear1.bias": (FEAT,)}
for l, k in ((0, 3 * J), (1, H)):
    shapes.update({f"recurrent.weight_ih_l{l}": (3 * H, k), f"recurrent.weight_hh_l{l}": (3 * H, H),
                   f"recurrent.bias_ih_l{l}": (3 * H,), f"recurrent.bias_hh_l{l}": (3 * H,)})
sd = {n: torch.from_numpy(synthetic.uniform(s, seed=100 + i, low=-0.15, high=0.15)) for i, (n, s) in enumerate(sorted(shapes.items()))}
pred = (0.4 * torch.from_numpy(synthetic.normal((B, S, T, J, 3), 11))).to(cuda)
target = (0.4 * torch.from_numpy(synthetic.normal((B, T, J, 3), 12))).to(cuda)

clf = metrics.FIDClassifier(sd, cuda)
acc = metrics.FIDAccumulator(clf)


class TorchOps(torch.nn.Module):
    """The reference classifier's layers as torch modules (fid_classifier.py:15-16, :43-53)."""

    def __init__(self):
        super().__init__()
        self.recurrent = torch.nn.GRU(3 * J, H, 2)
        self.linear1 = torch.nn.Linear(H, FEAT)

    def get_fid_features(self, motion_sequence):
        x = motion_sequence.permute(2, 0, 1).contiguous()
        h = torch.randn(2, x.size(1), H, device=x.device)
        o, _ = self.recurrent(x.float(), h)
        return torch.tanh(self.linear1(o[-1]))


ref = TorchOps()
ref.load_state_dict(sd)
ref = ref.to(cuda).eval()


def hip_batch():
    acc.update(pred, target)
    torch.cuda.synchronize()


@torch.no_grad()
def torch_batch():
    p = pred.reshape(*pred.shape[:-2], -1)
    p = p.reshape(-1, *p.shape[2:]).permute(0, 2, 1)
    t = target.reshape(*target.shape[:-2], -1).permute(0, 2, 1)
    a = ref.get_fid_features(p.float()).cpu().data.numpy()
    b = ref.get_fid_features(t.float()).cpu().data.numpy()
    return a, b


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


hip = timed(hip_batch)
tor = timed(torch_batch)

# the feature pass alone, by device events
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
h0 = torch.zeros(2, B * S, H, device=cuda)
ev[0].record()
f_hip = clf.features(pred, h0)
ev[1].record()
torch.cuda.synchronize()
feat_ms = ev[0].elapsed_time(ev[1])
with torch.no_grad():
    o, _ = ref.recurrent(pred.reshape(B * S, T, 3 * J).permute(1, 0, 2).contiguous(), h0)
    f_tor = torch.tanh(ref.linear1(o[-1]))
    n64 = min(B * S, 128)
    m64 = TorchOps().double()
    m64.load_state_dict({k: v.double() for k, v in sd.items()})
    o64, _ = m64.recurrent(pred[:, :, :, :, :].reshape(B * S, T, 3 * J)[:n64].cpu().double().permute(1, 0, 2).contiguous(),
                           torch.zeros(2, n64, H, dtype=torch.float64))
    f64 = torch.tanh(m64.linear1(o64[-1]))
flops = 2.0 * (B * S + B) * T * 3 * H * (3 * J + 3 * H)
print(json.dumps({
    "metric": "FID accumulation of one batch, wall ms (features of pred and target + statistics)",
    "shape": {"sequences": B, "samples": S, "frames": T, "joints": J}, "repeats": REPEATS, "warmup": WARMUP,
    "hip": hip, "torch_ops": tor, "ratio_torch_over_hip": tor["median_ms"] / hip["median_ms"],
    "spread": {"hip_ms": hip["max_ms"] - hip["min_ms"], "torch_ms": tor["max_ms"] - tor["min_ms"]},
    "hip_feature_pass_pred_device_ms": feat_ms, "gru_tflop_per_batch": flops / 1e12,
    "hip_feature_pass_tflops": 2.0 * B * S * T * 3 * H * (3 * J + 3 * H) / 1e12 / (feat_ms * 1e-3),
    "max_abs_hip_minus_torch_ops": float((f_hip - f_tor).abs().max()),
    "max_abs_hip_minus_float64": float((f_hip[:n64].cpu().double() - f64).abs().max()),
    "max_abs_torch_ops_minus_float64": float((f_tor[:n64].cpu().double() - f64).abs().max()),
    "device": torch.cuda.get_device_name(0)}))
