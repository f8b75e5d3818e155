"""Stage-1 training step of the graph-GRU autoencoder (reference
AutoEncoderTrainer.train_step, src/core/trainer.py:79-96): autoencode + L1 loss + backward +
clip_grad_norm_ + AdamW(amsgrad), B = 64 sequences, T_obs = 25, ph in {10, 50, 100}, J = 16 and 21,
with the GRUs on the HIP sequence path and, in the same process on the same GPU, with
training.set_hip_training(False) (the unrolled torch ops).  Per setting: warm-up steps, then the
median of `--reps` individually synchronised steps.  Also splits the decoder-shaped core call into
its phases (forward sweep, reverse sweep, batched gradients) by timing the entries directly.
Writes profiles/ae_train/bench.json and prints it.  --optimizer hip runs the tail of the step as
optim.FusedAdam(max_grad_norm=1) instead of clip_grad_norm_ + torch.optim.AdamW;
"torch,hip" times both in the one process (the result then carries a row per optimizer).
--arch lstm times the graph-LSTM autoencoder instead (StaticGraphLSTM encoder and decoder, DESIGN.md
§4r2; same shapes and method) and writes profiles/ae_train_lstm/bench.json.
Usage: python tools/bench_train_autoencoder.py [--arch gru] [--reps 9] [--warmup 3]
       [--out profiles/ae_train/bench.json] [--optimizer torch] [--shapes 16:10,16:50,...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from skeletondiffusion_amd import _lib, optim, synthetic, training  # noqa: E402
from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder  # noqa: E402
from skeletondiffusion_amd.skeletons import skeleton  # noqa: E402

SKEL = {16: "h36m16", 21: "amass21"}


ARCH = {"gru": "StaticGraphGRU", "lstm": "StaticGraphLSTM"}


def model(J, dev, arch="gru"):
    _, _, _, types = skeleton(SKEL[J])
    m = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=J, encoder_hidden_size=96, decoder_hidden_size=96,
                    latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                    recurrent_arch_enc=ARCH[arch], recurrent_arch_decoder=ARCH[arch], if_consider_hip=False)
    synthetic.fill_module_(m, 4321)
    return m.to(dev).train()


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def step_time(J, B, T_obs, ph, hip, warmup, reps, dev, optimizer="torch", arch="gru"):
    prev = training.set_hip_training(hip)
    try:
        m = model(J, dev, arch)
        fused = optimizer == "hip"
        opt = optim.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-2, amsgrad=True, decoupled_weight_decay=True,
                              max_grad_norm=1.0) if fused else torch.optim.AdamW(m.parameters(), lr=1e-4, amsgrad=True)
        past = torch.from_numpy(synthetic.normal((B, T_obs, J, 3), seed=51)).to(dev) * 0.3
        y = torch.from_numpy(synthetic.normal((B, ph, J, 3), seed=52)).to(dev) * 0.3

        def step():
            opt.zero_grad(set_to_none=True)
            out, _, _ = m.autoencode(y, past, ph)
            loss = m.loss(out, y)
            loss.backward()
            if not fused:
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()

        med, lo, hi = median_ms(step, warmup, reps)
    finally:
        training.set_hip_training(prev)
    return {"median_ms": med, "min_ms": lo, "max_ms": hi}


def core_phases(J, B, T, warmup, reps, dev):
    """The decoder-shaped core call (Ta = 1, Tg = T, H = 96) split by timing the entries: the
    forward sweep, the backward with no batched output asked for (the reverse sweep), and the full
    backward (batched gradients = the difference)."""
    H, L = 96, _lib.lib()
    _, _, _, types = skeleton(SKEL[J])
    nt = (ctypes.c_int64 * J)(*[int(t) for t in types])
    n_types = int(max(types)) + 1
    g = torch.Generator().manual_seed(3)
    f = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)  # noqa: E731
    a, h0, W, b = f(B, 1, J, 3 * H) * 0.5, f(B, J, H) * 0.5, f(n_types, 3 * H, H) / H ** 0.5, f(n_types, 3 * H) * 0.1
    gx = torch.nn.functional.normalize(torch.eye(J, device=dev) + f(T, J, J).abs() * 0.1, p=1., dim=2).contiguous()
    hs, hprev = torch.empty(B, T, J, H, device=dev), torch.empty(B, T, J, H, device=dev)
    c, gates = torch.empty(B, T, J, 3 * H, device=dev), torch.empty(B, T, J, 4 * H, device=dev)
    dhs = f(B, T, J, H)
    da, dh0, dgx = torch.empty_like(a), torch.empty_like(h0), torch.empty_like(gx)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    nbytes = L.sd_gru_train_workspace_bytes(B, T, J, H, n_types)
    ws = torch.empty((nbytes + 3) // 4, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def fwd():
        _lib.check(L.sd_gru_train_forward(a.data_ptr(), 1, h0.data_ptr(), gx.data_ptr(), T, W.data_ptr(), b.data_ptr(), nt,
                                          n_types, B, T, J, H, hs.data_ptr(), hprev.data_ptr(), c.data_ptr(),
                                          gates.data_ptr(), ws.data_ptr(), nbytes, s))

    def bwd(full):
        o = [t.data_ptr() if full else None for t in (da, dh0, dgx, dW, db)]
        _lib.check(L.sd_gru_train_backward(dhs.data_ptr(), a.data_ptr(), 1, gx.data_ptr(), T, W.data_ptr(), nt, n_types,
                                           hprev.data_ptr(), c.data_ptr(), gates.data_ptr(), B, T, J, H, *o, ws.data_ptr(),
                                           nbytes, s))

    t_f = median_ms(fwd, warmup, reps)[0]
    t_s = median_ms(lambda: bwd(False), warmup, reps)[0]
    t_b = median_ms(lambda: bwd(True), warmup, reps)[0]
    saved = (hprev.numel() + c.numel() + gates.numel()) * 4
    return {"forward_sweep_ms": t_f, "reverse_sweep_ms": t_s, "batched_gradients_ms": t_b - t_s,
            "saved_state_bytes": saved}


def lstm_core_phases(J, B, T, warmup, reps, dev):
    """`core_phases` for the LSTM entries (Ta = 1, Tg = T, H = 96)."""
    H, L = 96, _lib.lib()
    _, _, _, types = skeleton(SKEL[J])
    nt = (ctypes.c_int64 * J)(*[int(t) for t in types])
    n_types = int(max(types)) + 1
    g = torch.Generator().manual_seed(3)
    f = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)  # noqa: E731
    a, h0, s0 = f(B, 1, J, 4 * H) * 0.5, f(B, J, H) * 0.5, f(B, J, H) * 0.5
    W, b = f(n_types, 4 * H, H) / H ** 0.5, f(n_types, 4 * H) * 0.1
    gx = torch.nn.functional.normalize(torch.eye(J, device=dev) + f(T, J, J).abs() * 0.1, p=1., dim=2).contiguous()
    hs, sseq, s_last = torch.empty(B, T, J, H, device=dev), torch.empty(B, T, J, H, device=dev), torch.empty_like(s0)
    P, gates = torch.empty(B, T, J, 4 * H, device=dev), torch.empty(B, T, J, 4 * H, device=dev)
    dhs = f(B, T, J, H)
    da, dh0, ds0, dgx = torch.empty_like(a), torch.empty_like(h0), torch.empty_like(s0), torch.empty_like(gx)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    nbytes = L.sd_lstm_train_workspace_bytes(B, T, J, H, n_types)
    ws = torch.empty((nbytes + 3) // 4, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def fwd():
        _lib.check(L.sd_lstm_train_forward(a.data_ptr(), 1, h0.data_ptr(), s0.data_ptr(), gx.data_ptr(), T, W.data_ptr(),
                                           b.data_ptr(), nt, n_types, B, T, J, H, hs.data_ptr(), s_last.data_ptr(),
                                           P.data_ptr(), gates.data_ptr(), sseq.data_ptr(), ws.data_ptr(), nbytes, s))

    def bwd(full):
        o = [t.data_ptr() if full else None for t in (da, dh0, ds0, dgx, dW, db)]
        _lib.check(L.sd_lstm_train_backward(dhs.data_ptr(), 1, gx.data_ptr(), T, W.data_ptr(), nt, n_types, h0.data_ptr(),
                                            s0.data_ptr(), hs.data_ptr(), P.data_ptr(), gates.data_ptr(), sseq.data_ptr(),
                                            B, T, J, H, *o, ws.data_ptr(), nbytes, s))

    t_f = median_ms(fwd, warmup, reps)[0]
    t_s = median_ms(lambda: bwd(False), warmup, reps)[0]
    t_b = median_ms(lambda: bwd(True), warmup, reps)[0]
    saved = (P.numel() + gates.numel() + sseq.numel()) * 4
    return {"forward_sweep_ms": t_f, "reverse_sweep_ms": t_s, "batched_gradients_ms": t_b - t_s,
            "saved_state_bytes": saved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arch", default="gru", choices=sorted(ARCH), help="the recurrent cell of encoder and decoder")
    ap.add_argument("--out", default=None, help="default profiles/ae_train/bench.json (gru), profiles/ae_train_lstm/bench.json")
    ap.add_argument("--optimizer", default="torch", help="torch, hip, or torch,hip")
    ap.add_argument("--shapes", default="16:10,16:50,16:100,21:10,21:50,21:100", help="J:ph,...")
    a = ap.parse_args()
    assert a.reps >= 7
    lstm = a.arch == "lstm"
    out = a.out or os.path.join(REPO, "profiles", "ae_train_lstm" if lstm else "ae_train", "bench.json")
    phases = lstm_core_phases if lstm else core_phases
    optimizers = a.optimizer.split(",")
    assert all(o in ("torch", "hip") for o in optimizers), a.optimizer
    dev = torch.device("cuda:0")
    B, T_obs = 64, 25
    rows = []
    for J, ph in (tuple(int(v) for v in sh.split(":")) for sh in a.shapes.split(",")):
        for optimizer in optimizers:
            hip = step_time(J, B, T_obs, ph, True, a.warmup, a.reps, dev, optimizer, a.arch)
            tor = step_time(J, B, T_obs, ph, False, a.warmup, a.reps, dev, optimizer, a.arch)
            rows.append({"J": J, "B": B, "T_obs": T_obs, "ph": ph, "optimizer": optimizer, "hip": hip,
                         "torch_ops_same_gpu": tor, "speedup": tor["median_ms"] / hip["median_ms"],
                         "decoder_core_phases": phases(J, B, ph, a.warmup, a.reps, dev)})
            print(json.dumps(rows[-1]), flush=True)
    res = {"metric": ("graph-LSTM " if lstm else "") + "stage-1 autoencoder training step, ms (autoencode + L1 + backward + clip_grad_norm_ + AdamW amsgrad)",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "data": "synthetic poses, synthetic weights (synthetic.fill_module_ seed 4321)", "shapes": rows,
           "hip_faster_at_every_shape": all(r["speedup"] > 1.0 for r in rows)}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
