"""The best-of-k training step of the release recipe (train_pick_best_sample_among_k = 50, input_space,
batch 64: 3,200 rows), both forms in one process:
  full      best_of_k.pick_best_loss + backward + optim.FusedAdam: forward and backward over all b k rows;
  selected  best_of_k.pick_best_loss_selected + backward + optim.FusedAdam: all rows scored without
            autograd, forward and backward over the b chosen rows.
Synthetic weights (synthetic.fill_module_, the test builders), synthetic latents and poses.  Device
events after a warm-up, the two forms alternating; per form ms per step, torch.cuda.max_memory_allocated
and the split of a step into its phases (events between the phases, a run of its own), and
sd_q_sample_groups against the torch expression it replaces.  Prints one JSON line and writes it to
--out/bench_J<J>.json.
Usage: python tools/bench_best_of_k.py [--J 16] [--b 64] [--k 50] [--obs 25] [--pred 100] [--steps 10]
       [--warmup 3] [--repeats 3] [--out profiles/selected_step]"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from conftest import build_release_diffusion, golden  # noqa: E402
from skeletondiffusion_amd import optim, synthetic, training  # noqa: E402
from skeletondiffusion_amd.core import best_of_k as B  # noqa: E402
from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder  # noqa: E402
from skeletondiffusion_amd.skeletons import skeleton  # noqa: E402

SKELETON = {16: "h36m16", 17: "freeman17", 21: "amass21"}  # the release recipes' skeletons, by joint count


def autoencoder(J, dev):
    _, _, _, types = skeleton(SKELETON[J])
    m = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=J, encoder_hidden_size=96, decoder_hidden_size=96,
                    latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                    recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU",
                    if_consider_hip=False).eval()
    synthetic.fill_module_(m, 4321)
    return m.to(dev)


class Marks:
    """Device events between the phases of a step; ms per phase averaged over the steps recorded."""

    def __init__(self):
        self.steps = []

    def begin(self):
        self.cur = [("begin", self._event())]
        self.steps.append(self.cur)

    def __call__(self, name):
        self.cur.append((name, self._event()))

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def split(self):
        torch.cuda.synchronize()
        out = {}
        for marks in self.steps:
            for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
                out[name] = out.get(name, 0.0) + a.elapsed_time(b) / len(self.steps)
        return out


def full_step(d, opt, data, x_cond, k, kw, mark=None):
    """pick_best_loss + backward + FusedAdam; with `mark`, pick_best_loss's own body with an event
    after each phase."""
    opt.zero_grad(set_to_none=True)
    if mark is None:
        loss, _ = B.pick_best_loss(d, data, x_cond, k, **kw)
    else:
        rows, w, samples = d(data, x_cond=x_cond, n_train_samples=k)
        mark("scoring_forward")
        out_c, fut_c = B.to_comparison_space_train(samples, diff_input=data, past_seq=kw["past_seq"],
                                                   autoencoder=kw["autoencoder"], fut_seq=kw["fut_seq"],
                                                   space=kw["similarity_space"], x_cond=x_cond,
                                                   prediction_horizon=kw["prediction_horizon"])
        mark("decode")
        sel, _ = B.get_ksimilarity_loss(rows, out_c, fut_c, similarity_space=kw["similarity_space"],
                                        autoencoder=kw["autoencoder"])
        loss = (sel * w).mean()
        mark("selection")
    loss.backward()
    if mark is not None:
        mark("backward")
    opt.step()
    if mark is not None:
        mark("optimizer")
    return loss


def selected_step(d, opt, data, x_cond, k, kw, step, mark=None):
    opt.zero_grad(set_to_none=True)
    loss, _, _, _ = B._selected_passes(d, data, x_cond, k, seed=77, step=step, mark=mark, **kw)
    loss.backward()
    if mark is not None:
        mark("backward")
    opt.step()
    if mark is not None:
        mark("optimizer")
    return loss


def time_steps(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--J", type=int, default=16, choices=sorted(SKELETON))
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--obs", type=int, default=25)
    ap.add_argument("--pred", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "selected_step"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_best_of_k: no HIP device (this benchmark has no CPU form)")
    dev = torch.device("cuda:0")
    J, b, k = a.J, a.b, a.k
    z = golden(f"release_{SKELETON[J]}_T10")
    ae = autoencoder(J, dev)
    data = torch.from_numpy(synthetic.uniform((b, J, 96), 61)).to(dev)
    x_cond = torch.from_numpy(synthetic.uniform((b, J, 96), 62)).to(dev)
    past = torch.from_numpy(synthetic.normal((b, a.obs, J, 3), 63) * 0.2).float().to(dev)
    fut = torch.from_numpy(synthetic.normal((b, a.pred, J, 3), 64) * 0.2).float().to(dev)
    kw = dict(similarity_space="input_space", autoencoder=ae, past_seq=past, fut_seq=fut, prediction_horizon=a.pred)

    forms = {}
    for name in ("full", "selected"):
        d = build_release_diffusion(z, device=dev).train()
        opt = optim.FusedAdam(d.model.parameters(), lr=1e-4)
        if name == "full":
            forms[name] = (lambda i, mark=None, d=d, opt=opt: full_step(d, opt, data, x_cond, k, kw, mark))
        else:
            forms[name] = (lambda i, mark=None, d=d, opt=opt: selected_step(d, opt, data, x_cond, k, kw, i, mark))
    res = {name: {"ms_per_step_runs": []} for name in forms}
    for name, fn in forms.items():
        for i in range(a.warmup):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(a.repeats):  # the two forms alternate
        for name, fn in forms.items():
            res[name]["ms_per_step_runs"].append(time_steps(fn, a.steps))
    for name, fn in forms.items():
        r = res[name]
        r["ms_per_step"] = min(r["ms_per_step_runs"])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn(0)
        torch.cuda.synchronize()
        r["max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
        marks = Marks()
        for i in range(a.steps):
            marks.begin()
            fn(i, marks)
        r["split_ms"] = marks.split()
        r["split_ms_total"] = sum(r["split_ms"].values())

    # the forward process alone: the kernel against the torch expression it replaces
    d = build_release_diffusion(z, device=dev)
    t = torch.randint(0, d.num_timesteps, (b,), device=dev)

    def q_hip(i):
        training.q_sample_groups(data, t, d.sqrt_alphas_cumprod, k, M=d.Umm_sqrt_Lambda_bar_t, seed=5, step=i,
                                 return_noise=True)

    def q_torch(i):
        xs, tt = data.repeat_interleave(k, dim=0), t.repeat_interleave(k, dim=0)
        d.q_sample(x_start=xs, t=tt, noise=d.get_white_noise(xs, tt))

    for fn in (q_hip, q_torch):
        time_steps(fn, 5)
    q = {"sd_q_sample_groups_ms": min(time_steps(q_hip, 50) for _ in range(3)),
         "torch_expression_ms": min(time_steps(q_torch, 50) for _ in range(3)),
         "bytes_written": 2 * b * k * J * 96 * 4}

    out = {"metric": "best-of-k training step, ms per step (loss + backward + FusedAdam)", "J": J, "b": b, "k": k,
           "rows": b * k, "obs": a.obs, "pred": a.pred, "T": int(z["T"]), "similarity_space": "input_space",
           "data": "synthetic latents and poses, release Denoiser and autoencoder with synthetic weights",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "full": res["full"], "selected": res["selected"],
           "speedup": res["full"]["ms_per_step"] / res["selected"]["ms_per_step"],
           "memory_ratio": res["selected"]["max_memory_allocated"] / res["full"]["max_memory_allocated"],
           "q_sample": q}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"bench_J{J}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
