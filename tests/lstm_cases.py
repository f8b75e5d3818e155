"""Shared cases of the graph-LSTM autoencoder tests (tests/test_lstm_autoencoder.py on the CPU,
tests/test_gpu_lstm_train.py on the device, tests/golden/gen_golden_lstm.py for the fixture).

`core_ref` is the float64-capable restatement of the LSTM sequence core (reference recurrent.py:
126-167 from the unmixed input projections, clockwork off): the role `core_ref` plays in
tests/test_gpu_gru_train.py.  The module recipe (sizes, seeds, inputs, the weight scale of the
second fixture set) is stated once here, so the generator and both consumers agree."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from skeletondiffusion_amd import synthetic
from skeletondiffusion_amd.skeletons import skeleton

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm.npz")

LSTM, GRU = "StaticGraphLSTM", "StaticGraphGRU"
ARCHS = {"ll": (LSTM, LSTM), "lg": (LSTM, GRU), "gl": (GRU, LSTM)}   # (encoder, decoder)
N_KEYS = {"ll": 33, "lg": 30, "gl": 30}
AE_SEED = 4321
# The second LSTM/LSTM set: weight_ih / weight_hh of both cells times SCALE after the synthetic
# fill.  The plain fill leaves every gate near its linear range; at this scale the generator
# measured (and asserts) max |Q| >= 2 over both sequences and a decoded maximum >= 0.3.
SCALE = 6.0
PH = 12
GRAD_WHOLE = 1024    # a gradient of at most this many entries is kept whole (every G, G_add and linear bias)
GRAD_SAMPLES = 256   # entries kept of a larger one (flat stride), beside the whole tensor's sum and norm


def ae_kwargs(J, arch_enc, arch_dec):
    return dict(num_nodes=J, encoder_hidden_size=96, decoder_hidden_size=96, latent_size=96, input_size=3,
                z_activation="tanh", enc_num_layers=1, output_size=3, recurrent_arch_enc=arch_enc,
                recurrent_arch_decoder=arch_dec, if_consider_hip=False)


def fill(m, scale=1.0):
    """The synthetic fill, then the recurrent weights of both cells times `scale`."""
    synthetic.fill_module_(m, AE_SEED)
    if scale != 1.0:
        with torch.no_grad():
            for rnn in (m.encoder.rnn, m.decoder.rnn):
                for cell in rnn.layers:
                    cell.weight_ih.mul_(scale)
                    cell.weight_hh.mul_(scale)
    return m


def make_model(arch, skel="h36m16", device="cpu", dtype=torch.float32, scale=1.0):
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    _, _, _, types = skeleton(skel)
    m = AutoEncoder(node_types=torch.from_numpy(types), **ae_kwargs(len(types), *ARCHS[arch])).eval()
    return fill(m, scale).to(device=device, dtype=dtype)


def fixture_inputs():
    """past (3, 30, 16, 3), latents (12, 16, 96), future (3, PH, 16, 3) of the fixture, float32."""
    past = torch.from_numpy(synthetic.normal((3, 30, 16, 3), seed=41)) * 0.3
    lat = torch.from_numpy(synthetic.uniform((12, 16, 96), seed=42))
    y = torch.from_numpy(synthetic.normal((3, PH, 16, 3), seed=43)) * 0.3
    return past, lat, y


def encode(m, past):
    """z_activation(encoder(past)) through the module's own forward (any device, any dtype)."""
    with torch.no_grad():
        return m.z_activation(m(past))


def decode(m, past, lat, ph=PH):
    """The decoder's forward on 4 latents per past sequence, no_grad (AutoEncoder.decode's semantics)."""
    with torch.no_grad():
        return m.decoder(x=past.repeat_interleave(4, 0)[:, -2:], h=lat, z=None, ph=ph)[0]


def grad_sample(g):
    """What the fixture keeps of one gradient tensor: all of it up to GRAD_WHOLE entries, GRAD_SAMPLES
    strided entries of a larger one; the sum; the L2 norm."""
    flat = g.detach().double().reshape(-1)
    stride = 1 if flat.numel() <= GRAD_WHOLE else -(-flat.numel() // GRAD_SAMPLES)
    return flat[::stride].clone(), flat.sum(), flat.square().sum().sqrt()


def train_step_grads(m, y, past, ph):
    m.zero_grad(set_to_none=True)
    out, z_past, z = m.autoencode(y, past, ph)
    loss = m.loss(out, y)
    loss.backward()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    return out.detach(), z_past.detach(), z.detach(), loss.detach(), grads


# ---- the sequence core ------------------------------------------------------------------------------

def core_ref(a, h0, s0, gx, W, b, types, T):
    """recurrent.py:126-167 from the unmixed input projections a = W_ih x, any dtype:
    P = a + W_hh h + b_hh, Q = gx P, chunks i | f | g | o.  Returns (hs (B, T, J, H), s_T)."""
    H = h0.shape[-1]
    Wj = W[types] if types is not None else W                                  # (J, 4H, H) or (4H, H)
    bj = (b[types] if types is not None else b) if b is not None else 0.0
    h, s, hs = h0, s0, []
    for t in range(T):
        g = gx[t if gx.shape[0] > 1 else 0]
        at = a[:, t if a.shape[1] > 1 else 0]
        P = at + (torch.einsum("jnk,bjk->bjn", Wj, h) if types is not None else h @ Wj.t()) + bj
        Q = g @ P
        i, f = torch.sigmoid(Q[..., :H]), torch.sigmoid(Q[..., H:2 * H])
        c, o = torch.tanh(Q[..., 2 * H:3 * H]), torch.sigmoid(Q[..., 3 * H:])
        s = f * s + i * c
        h = o * torch.tanh(s)
        hs.append(h)
    return torch.stack(hs, 1), s


def core_inputs(J, H, B, T, Ta, Tg, typed, bias, seed):
    """`core_inputs` of tests/test_gpu_gru_train.py with four gate blocks, plus a random s0."""
    g = torch.Generator().manual_seed(seed)
    n_types = max(2, J // 2) if typed else 0
    types = (torch.arange(J) * 3 + 1) % n_types if typed else None             # repeated types
    lead = (n_types,) if typed else ()
    G = torch.eye(J) + torch.rand(Tg, J, J, generator=g) * 0.1
    return dict(a=torch.randn(B, Ta, J, 4 * H, generator=g) * 0.5, h0=(torch.rand(B, J, H, generator=g) * 2 - 1) * 0.5,
                gx=F.normalize(G, p=1., dim=2), W=(torch.rand(*lead, 4 * H, H, generator=g) * 2 - 1) / H ** 0.5,
                b=(torch.rand(*lead, 4 * H, generator=g) * 2 - 1) * 0.1 if bias else None, types=types,
                w=torch.randn(B, T, J, H, generator=g), s0=torch.randn(B, J, H, generator=g) * 0.5)


CORE_NAMES = ("a", "h0", "s0", "gx", "W", "b")


def run_core(inp, T, dtype=None, device=None, hip=False):
    from skeletondiffusion_amd import training

    names = [k for k in CORE_NAMES if inp[k] is not None]
    x = {k: inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    types = inp["types"]
    if hip:
        hs, s_last = training.graph_lstm(x["a"], x["h0"], x["s0"], x["gx"], x["W"], x.get("b"), types, steps=T)
    else:
        hs, s_last = core_ref(x["a"], x["h0"], x["s0"], x["gx"], x["W"], x.get("b"), types, T)
    (hs * inp["w"].to(hs)).sum().backward()
    return hs.detach(), s_last.detach(), {k: x[k].grad for k in names}


CORE_CASES = [  # (J, H, B, T, Ta, Tg, typed weights, bias)
    (16, 96, 5, 7, 7, 1, True, True),      # the encoder's form
    (21, 96, 1, 1, 1, 1, False, False),    # one row, one step, shared weights, no bias
    (17, 32, 37, 2, 1, 2, True, True),     # the decoder's form; rows off every tile
    (16, 96, 33, 9, 9, 9, False, True),    # a projection and a matrix per step
    (17, 32, 37, 2, 2, 1, True, False),    # per-frame projections, one matrix, no bias
    (64, 16, 2, 3, 3, 3, True, True),      # node limit
    (3, 256, 9, 2, 1, 1, False, True),     # width limit
]


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)
