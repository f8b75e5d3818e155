"""End-to-end evaluation pipeline on one MI355X (the reference's get_prediction,
eval_prepare_model.py:89-121): past embedding (HIP encoder) -> sample() of 50 futures per
sequence (HIP sampler, release Denoiser) -> decode to 120 frames (HIP decoder) -> APD / ADE / FDE
(HIP metrics), on synthetic weights and data of the AMASS shape (J = 21, 30 observed frames,
T = 10 as the release config).  Prints one JSON line with per-stage times and end-to-end futures/s,
next to the reference's published end-to-end rate (12,726 AMASS test segments x 50
futures in ~12 min on an RTX6000 ~ 884 futures/s; data loading included there).

With --long-term FACTOR the line also carries the long-term rollout (the reference's
long_term_prediction_best_every50, eval_utils.py:44-67, through skeletondiffusion_amd.evaluation):
ceil(FACTOR) segments of 50 futures x 120 frames, the future closest to the ground truth kept and its
last 30 frames fed back, with per-segment stage times and the total.

With --realism the fused body-realism / limb-angle / motion-profile call (metrics.realism)
runs after the existing metrics on the same decoded futures, and its milliseconds are reported.

With --fid the pipeline runs at the H36M shape the FID classifier is trained for (J = 16, 25 observed and 100
predicted frames) and ends with the FID accumulation (metrics.FIDAccumulator, DESIGN.md §4p: the classifier's
features of the 50 futures and of the ground truth, folded into the running statistics) on synthetic
classifier weights; its milliseconds and the FID value are reported.

Usage: python tools/eval_pipeline.py [sequences] [T] [--long-term FACTOR] [--realism] [--fid]"""
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from bench import build_config  # noqa: E402
from skeletondiffusion_amd import evaluation, metrics, skeletons, synthetic  # noqa: E402
from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder  # noqa: E402
from skeletondiffusion_amd.skeletons import skeleton  # noqa: E402

ARGS = sys.argv[1:]
REALISM = "--realism" in ARGS
if REALISM:
    ARGS.remove("--realism")
FID = "--fid" in ARGS
if FID:
    ARGS.remove("--fid")
LONG_TERM = None
if "--long-term" in ARGS:
    _i = ARGS.index("--long-term")
    LONG_TERM = float(ARGS[_i + 1])
    del ARGS[_i:_i + 2]
NSEQ = int(ARGS[0]) if len(ARGS) > 0 else 256
T = int(ARGS[1]) if len(ARGS) > 1 else 10
FUT, OBS, PH = (50, 25, 100) if FID else (50, 30, 120)
SKEL = "h36m16" if FID else "amass21"
cuda = torch.device("cuda:0")
d, _, _ = build_config("amass16" if FID else "amass21", cuda, T=T, batch=1, futures=FUT)
_, _, _, types = skeleton(SKEL)
J = len(types)
ae = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=J, encoder_hidden_size=96, decoder_hidden_size=96,
                 latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                 recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU",
                 if_consider_hip=False).eval()
synthetic.fill_module_(ae, 4321)
ae = ae.to(cuda)
obs = (torch.from_numpy(synthetic.normal((NSEQ, OBS, J, 3), seed=51)) * 0.3).to(cuda)
target = (torch.from_numpy(synthetic.normal((NSEQ, PH, J, 3), seed=52)) * 0.3).to(cuda)
fid_acc = None
if FID:  # tests/golden/gen_golden_fid.py's weight recipe: unsaturated activations
    _shapes = {"linear1.weight": (30, 128), "linear1.bias": (30,)}
    for _l, _k in ((0, 3 * J), (1, 128)):
        _shapes.update({f"recurrent.weight_ih_l{_l}": (384, _k), f"recurrent.weight_hh_l{_l}": (384, 128),
                        f"recurrent.bias_ih_l{_l}": (384,), f"recurrent.bias_hh_l{_l}": (384,)})
    fid_acc = metrics.FIDAccumulator(metrics.FIDClassifier(
        {n: torch.from_numpy(synthetic.uniform(s, seed=100 + i, low=-0.15, high=0.15)) for i, (n, s) in enumerate(sorted(_shapes.items()))},
        cuda))


def run():
    st = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    ev[0].record()
    z_past = ae.get_past_embedding(obs)
    ev[1].record()
    lat, _ = d.sample(batch_size=NSEQ * FUT, x_cond=z_past, seed=7)
    ev[2].record()
    pred = ae.decode(obs.repeat_interleave(FUT, 0), lat, z_past.repeat_interleave(FUT, 0), ph=PH)
    ev[3].record()
    p = pred.view(NSEQ, FUT, PH, J, 3)
    apd = metrics.apd(p)
    ade = metrics.ade(target, p)
    fde = metrics.fde(target, p)
    ev[4].record()
    real = metrics.realism(p, target, skeletons.limbseq(SKEL), skeletons.limb_angles_idx(SKEL)) if REALISM else None
    ev[5].record()
    if FID:
        fid_acc.reset()
        fid_acc.update(p, target)
    ev[6].record()
    torch.cuda.synchronize()
    for k, (a, b) in zip(("encode", "sample", "decode", "metrics"), zip(ev, ev[1:])):
        st[k] = a.elapsed_time(b)
    if REALISM:
        st["realism"] = ev[4].elapsed_time(ev[5])
        st["realism_values"] = {"MAE": float(real.mae.mean()), "StretchMean": 100 * float(real.smean_mean.mean()),
                                "JitterMean": 100 * float(real.jmean_mean.mean()),
                                "StretchRMSE": 100 * float(real.srmse_std_mean.mean()),
                                "JitterRMSE": 100 * float(real.jrmse_std_mean.mean()),
                                "motion_mean": float(real.motion.mean())}
    if FID:
        st["fid"] = ev[5].elapsed_time(ev[6])
        st["fid_value"] = fid_acc.compute()
    return st, float(apd.mean()), float(ade.mean()), float(fde.mean())


def run_long_term(factor):
    """best_every50 on the same setup: (per-segment stage ms, device ms of the rollout, mpjpe of the
    returned trajectory against the long target)."""
    frames = int(factor * PH)
    long_target = (torch.from_numpy(synthetic.normal((NSEQ, frames, J, 3), seed=53)) * 0.3).to(cuda)
    marks = []

    def predict(past, **kwargs):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        lat, z_past = evaluation.get_diffusion_latent_codes(past, (ae, d), num_samples=FUT, sampler_kwargs={"seed": 7})
        ev[1].record()
        pred = evaluation.decode_latent_pred(past, lat, z_past, (ae, d), num_samples=FUT, pred_length=PH)
        ev[2].record()
        marks.append(ev)
        return pred

    _, pred, _, _ = evaluation.long_term_prediction_best_every50(
        obs, long_target, None, predict, num_samples=FUT, config={"long_term_factor": factor, "pred_length": PH})
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    torch.cuda.synchronize()
    segs = []
    for k, ev in enumerate(marks):  # the selection runs from a segment's decode to the next segment's start
        nxt = marks[k + 1][0] if k + 1 < len(marks) else end
        segs.append({"encode_sample": ev[0].elapsed_time(ev[1]), "decode": ev[1].elapsed_time(ev[2]),
                     "select": ev[2].elapsed_time(nxt)})
    mp = metrics.mpjpe(long_target, pred[:, :1])
    return segs, marks[0][0].elapsed_time(end), float(mp.mean()), frames


run()  # warm-up: plans, graphs, workspaces
t0 = time.perf_counter()
st, apd, ade, fde = run()
wall = time.perf_counter() - t0
rows = NSEQ * FUT
extra = {}
if LONG_TERM is not None:
    run_long_term(LONG_TERM)  # warm-up: the last segment's shapes
    t0 = time.perf_counter()
    segs, dev_ms, mp, frames = run_long_term(LONG_TERM)
    extra = {"long_term": {"factor": LONG_TERM, "segments": len(segs), "frames": frames, "segment_stage_ms": segs,
                           "device_ms": dev_ms, "wall_ms": (time.perf_counter() - t0) * 1e3,
                           "futures_per_s": rows * len(segs) / (dev_ms * 1e-3), "mpjpe_best": mp}}
print(json.dumps({"metric": "end-to-end evaluated futures/s (encode + sample + decode + APD/ADE/FDE)",
                  "value": rows / wall, "unit": "futures/s", "sequences": NSEQ, "futures": FUT, "J": J, "T": T,
                  "obs_frames": OBS, "pred_frames": PH, "wall_ms": wall * 1e3, "stage_ms": st,
                  "apd": apd, "ade": ade, "fde": fde, "data": "synthetic weights and motions",
                  "reference_published": {"value": 884, "unit": "futures/s end-to-end",
                                          "hardware": "NVIDIA RTX6000", "source": "BASELINE.md (README.md:223)"},
                  **extra}))
