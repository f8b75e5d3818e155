#!/usr/bin/env python3
"""Generate tests/golden/lstm.npz by running the REFERENCE's AutoEncoder with StaticGraphLSTM
encoders / decoders on the CPU (src/core/network/nn/{autoencoder,encoder,decoder}.py,
src/core/network/layers/recurrent.py:13-203).

Build-container tool only, like gen_golden.py (imported here for its third-party shim and path
setup): it imports the read-only reference tree and no test uses it.  Only data is written: the
sorted state-dict keys, reference outputs and gradient samples.  Weights and inputs are regenerated
from their seeds by the consumers (tests/lstm_cases.py states the recipe once, for both sides).

Sets, all at the release sizes (H36M 16-joint node types, H = L = 96, F = 3), synthetic fill 4321:
  ll, lg, gl   encoder / decoder = LSTM/LSTM, LSTM/GRU, GRU/LSTM
  lls          LSTM/LSTM with weight_ih / weight_hh of both cells times lstm_cases.SCALE: the plain
               fill leaves the gates almost linear, where a wrong gate order or a dropped forget path
               could hide inside the tolerances.  Asserted and recorded here: the largest mixed
               pre-activation |Q| over both sequences is >= 2 and the decoded maximum is >= 0.3.
Per set: z_past of 3 x 30 observed frames, decode of 3 x 4 latents for 12 frames, autoencode's output,
z and L1 loss at ph = 12, from the float64 module (the reference's float32 module is within 1.4e-7 of
these everywhere, measured when this was written; the float32 consumers compare against them).
For ll and lls also the float64 gradient of every parameter after loss.backward(): per parameter
(sorted names `*_gnames`, None gradients listed in `*_gnone`) the whole tensor when it has at most
lstm_cases.GRAD_WHOLE entries (every G, G_add and linear bias), else lstm_cases.GRAD_SAMPLES strided
entries (`*_g/<name>`), and always the sum and the L2 norm of the whole tensor (`*_gsum`, `*_gnorm`).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lstm.py
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gen_golden  # noqa: E402,F401  (the reference's import path and the third-party shim)
import lstm_cases as C  # noqa: E402
from skeletondiffusion_amd.skeletons import skeleton  # noqa: E402
from src.core.network.nn.autoencoder import AutoEncoder  # noqa: E402


class QProbe:
    """Largest |Q| = |gx (W_ih x + W_hh h + b_hh)| any LSTM cell of the module sees (recomputed from
    the cell's inputs in a forward pre-hook)."""

    def __init__(self, m):
        self.max = 0.0
        for rnn in (m.encoder.rnn, m.decoder.rnn):
            for cell in rnn.layers:
                if cell.weight_hh.shape[-2] == 4 * cell.hidden_size:
                    cell.register_forward_pre_hook(self.hook)

    def hook(self, cell, args):
        x, (hx, _, gx) = args[0], args[1]
        with torch.no_grad():
            if gx is None:
                gx = F.normalize(cell.G, p=1., dim=1)
            idx = cell.node_type_index
            P = torch.einsum("jnk,bjk->bjn", cell.weight_ih[idx], x) + torch.einsum("jnk,bjk->bjn", cell.weight_hh[idx], hx)
            self.max = max(self.max, float((gx @ (P + cell.bias_hh[idx])).abs().max()))


def run_set(tag, arch, scale, with_grads, out):
    _, _, _, types = skeleton("h36m16")
    past, lat, y = (v.double() for v in C.fixture_inputs())
    m = AutoEncoder(node_types=torch.from_numpy(types), **C.ae_kwargs(16, *C.ARCHS[arch])).eval()
    m = C.fill(m, scale).double()
    probe = QProbe(m)
    with torch.no_grad():
        z_past = m.get_past_embedding(past)
        dec = m.decode(past.repeat_interleave(4, 0), lat, z_past.repeat_interleave(4, 0), ph=C.PH)
    ae_out, _, z = m.autoencode(y, past, ph=C.PH)
    loss = m.loss(ae_out, y)
    out.update({f"{tag}_z_past": z_past.numpy(), f"{tag}_dec": dec.numpy(), f"{tag}_ae_out": ae_out.detach().numpy(),
                f"{tag}_ae_z": z.detach().numpy(), f"{tag}_ae_loss": loss.detach().numpy(),
                f"{tag}_keys": np.array(sorted(m.state_dict().keys())), f"{tag}_qmax": np.float64(probe.max),
                f"{tag}_decmax": np.float64(dec.abs().max())})
    print(f"{tag}: {len(m.state_dict())} keys, max|Q| {probe.max:.3f}, max|dec| {float(dec.abs().max()):.3f}, "
          f"loss {float(loss.detach()):.6f}")
    if not with_grads:
        return
    loss.backward()
    params = dict(m.named_parameters())
    have = [n for n in sorted(params) if params[n].grad is not None]
    out[f"{tag}_gnames"] = np.array(have)
    out[f"{tag}_gnone"] = np.array([n for n in sorted(params) if params[n].grad is None])
    sums, norms = [], []
    for n in have:
        smp, s, nrm = C.grad_sample(params[n].grad)
        out[f"{tag}_g/{n}"] = smp.numpy()
        sums.append(float(s))
        norms.append(float(nrm))
    out[f"{tag}_gsum"], out[f"{tag}_gnorm"] = np.array(sums), np.array(norms)


def main():
    out = {"scale": np.float64(C.SCALE)}
    for tag in ("ll", "lg", "gl"):
        run_set(tag, tag, 1.0, tag == "ll", out)
        assert len(out[f"{tag}_keys"]) == C.N_KEYS[tag]
    run_set("lls", "ll", C.SCALE, True, out)
    assert float(out["lls_qmax"]) >= 2.0, out["lls_qmax"]
    assert float(out["lls_decmax"]) >= 0.3, out["lls_decmax"]
    np.savez_compressed(C.GOLDEN, **out)
    print(f"wrote {C.GOLDEN}: {os.path.getsize(C.GOLDEN) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
