"""Stage-1 training of the graph-GRU autoencoder on HIP: the sequence core
(`training.graph_gru`), the gx table (`training.gx_table`) and the whole module's
autoencode + loss + backward against float64 on the CPU.

Gradient yardstick, per tensor: err = max|g - g64| / max|g64| (no absolute floor) with g64 the
torch-op path in float64 on the CPU, and the bound err_hip <= 8 x err_torch32, err_torch32 being
the same torch-op path in float32 on the CPU for the same tensor and inputs, computed here.  The
factor covers the different summation order over the B T rows and the device sigmoid / tanh
compounded over the steps.  A tensor whose float64 gradient is identically zero must be exactly
zero."""
import pytest
import torch
import torch.nn.functional as F

import oracle as O
from skeletondiffusion_amd import synthetic, training
from skeletondiffusion_amd.skeletons import skeleton

FACTOR = 8.0
FWD_TOL = 1e-5   # forward of the core / the table
OUT_TOL = 1e-4   # decoded frames (tests/test_autoencoder.py)


def rel_err(g, g64):
    g, g64 = g.detach().double().cpu(), g64.detach().double().cpu()
    den = float(g64.abs().max()) if g64.numel() else 0.0
    if den == 0.0:
        return 0.0 if (g.numel() == 0 or float(g.abs().max()) == 0.0) else float("inf")
    return float((g - g64).abs().max()) / den


def assert_bound(name, g_hip, g32, g64, report):
    e_hip, e_32 = rel_err(g_hip, g64), rel_err(g32, g64)
    report.append(f"{name}: err_hip {e_hip:.3e} err_torch32 {e_32:.3e} ratio {e_hip / e_32 if e_32 else float('nan'):.2f}")
    print(report[-1])
    assert e_hip <= FACTOR * e_32, report[-1]


# ---- the core against a torch restatement -------------------------------------------------------

def core_ref(a, h0, gx, W, b, types, T):
    """recurrent.py:321-366 from the unmixed input projections, any dtype."""
    H = h0.shape[-1]
    Wj = W[types] if types is not None else W                                  # (J, 3H, H) or (3H, H)
    bj = (b[types] if types is not None else b) if b is not None else 0.0
    h, hs = h0, []
    for t in range(T):
        g = gx[t if gx.shape[0] > 1 else 0]
        at = a[:, t if a.shape[1] > 1 else 0]
        c = (torch.einsum("jnk,bjk->bjn", Wj, h) if types is not None else h @ Wj.t()) + bj
        X, Hh = g @ at, g @ c
        r = torch.sigmoid(X[..., :H] + Hh[..., :H])
        z = torch.sigmoid(X[..., H:2 * H] + Hh[..., H:2 * H])
        n = torch.tanh(X[..., 2 * H:] + r * Hh[..., 2 * H:])
        h = n - n * z + z * h
        hs.append(h)
    return torch.stack(hs, 1)


def core_inputs(J, H, B, T, Ta, Tg, typed, bias, seed):
    g = torch.Generator().manual_seed(seed)
    n_types = max(2, J // 2) if typed else 0
    types = (torch.arange(J) * 3 + 1) % n_types if typed else None             # repeated types
    lead = (n_types,) if typed else ()
    G = torch.eye(J) + torch.rand(Tg, J, J, generator=g) * 0.1
    return dict(a=torch.randn(B, Ta, J, 3 * H, generator=g) * 0.5, h0=(torch.rand(B, J, H, generator=g) * 2 - 1) * 0.5,
                gx=F.normalize(G, p=1., dim=2), W=(torch.rand(*lead, 3 * H, H, generator=g) * 2 - 1) / H ** 0.5,
                b=(torch.rand(*lead, 3 * H, generator=g) * 2 - 1) * 0.1 if bias else None, types=types,
                w=torch.randn(B, T, J, H, generator=g))


def run_core(inp, T, dtype=None, device=None, hip=False):
    names = [k for k in ("a", "h0", "gx", "W", "b") if inp[k] is not None]
    x = {k: inp[k].detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    types = inp["types"]
    if hip:
        hs = training.graph_gru(x["a"], x["h0"], x["gx"], x["W"], x.get("b"), types, steps=T)
    else:
        hs = core_ref(x["a"], x["h0"], x["gx"], x["W"], x.get("b"), types, T)
    (hs * inp["w"].to(hs)).sum().backward()
    return hs.detach(), {k: x[k].grad for k in names}


CORE_CASES = [  # (J, H, B, T, Ta, Tg, typed weights, bias)
    (16, 96, 5, 7, 7, 1, True, True),      # the encoder's form
    (21, 96, 1, 1, 1, 1, False, False),    # one row, one step, shared weights, no bias
    (17, 32, 37, 2, 1, 2, True, True),     # the decoder's form; rows not a multiple of any tile
    (16, 96, 33, 9, 9, 9, False, True),    # a projection and a matrix per step
    (17, 32, 37, 2, 2, 1, True, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("J,H,B,T,Ta,Tg,typed,bias", CORE_CASES)
def test_core_matches_float64(J, H, B, T, Ta, Tg, typed, bias, cuda):
    inp = core_inputs(J, H, B, T, Ta, Tg, typed, bias, seed=J * 1000 + B)
    hs64, g64 = run_core(inp, T, dtype=torch.float64)
    _, g32 = run_core(inp, T, dtype=torch.float32)
    hs, g = run_core(inp, T, dtype=torch.float32, device=cuda, hip=True)
    torch.cuda.synchronize()
    assert hs.shape == (B, T, J, H)
    assert float((hs.double().cpu() - hs64).abs().max()) < FWD_TOL
    report = []
    for k in g64:
        assert g[k].shape == inp[k].shape
        assert_bound(f"core {(J, H, B, T, Ta, Tg)} d{k}", g[k], g32[k], g64[k], report)


@pytest.mark.gpu
def test_core_empty_batch(cuda):
    inp = core_inputs(16, 96, 0, 3, 3, 1, True, True, seed=1)
    hs, g = run_core(inp, 3, dtype=torch.float32, device=cuda, hip=True)
    torch.cuda.synchronize()
    assert hs.shape == (0, 3, 16, 96)
    for k in ("gx", "W", "b"):
        assert g[k].shape == inp[k].shape and float(g[k].abs().max()) == 0.0
    assert g["a"].shape == (0, 3, 16, 288) and g["h0"].shape == (0, 16, 96)


# ---- the gx table ---------------------------------------------------------------------------------

def gxt_ref(G, G_add, T):
    gx, out = F.normalize(G, p=1., dim=1), []
    for _ in range(T):
        out.append(gx)
        gx = F.normalize(gx + G_add, p=1., dim=1)
    return torch.stack(out)


@pytest.fixture(scope="module")
def gx_params():
    """G / G_add of a filled cell per J, checked away from the abs kink of the L1 norm."""
    from skeletondiffusion_amd.core.network.autoencoder import StaticGraphGRUCell

    out = {}
    for J in (16, 21, 51):
        cell = StaticGraphGRUCell(4, 16, num_nodes=J, learn_influence=True, learn_additive_graph_influence=True)
        synthetic.fill_module_(cell, 4321)
        G, A = cell.G.detach().clone(), cell.G_add.detach().clone()
        gx = gxt_ref(G.double(), A.double(), 31)
        assert float((gx + A.double()).abs().min()) > 1e-6
        out[J] = (G, A)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 30])
@pytest.mark.parametrize("J", [16, 21, 51])
def test_gx_table_matches_float64(J, T, gx_params, cuda):
    G, A = gx_params[J]
    w = torch.randn(T, J, J, generator=torch.Generator().manual_seed(J + T))

    def run(dtype, device=None, hip=False):
        g, a = (v.detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for v in (G, A))
        out = training.gx_table(g, a, T) if hip else gxt_ref(g, a, T)
        (out * w.to(out)).sum().backward()
        return out.detach(), g.grad, (a.grad if a.grad is not None else torch.zeros_like(a))

    o64, dG64, dA64 = run(torch.float64)
    _, dG32, dA32 = run(torch.float32)
    o, dG, dA = run(torch.float32, cuda, hip=True)
    torch.cuda.synchronize()
    assert o.shape == (T, J, J) and float((o.double().cpu() - o64).abs().max()) < FWD_TOL
    report = []
    assert_bound(f"gx table J={J} T={T} dG", dG, dG32, dG64, report)
    assert_bound(f"gx table J={J} T={T} dG_add", dA, dA32, dA64, report)


# ---- the whole module -------------------------------------------------------------------------------

def make_model(skel, device="cpu", dtype=torch.float32):
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    _, _, _, types = skeleton(skel)
    J = len(types)
    m = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=J, encoder_hidden_size=96, decoder_hidden_size=96,
                    latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                    recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU", if_consider_hip=False)
    synthetic.fill_module_(m, 4321)
    return m.to(device=device, dtype=dtype), types


def module_inputs(J, B, T_obs, ph):
    past = torch.from_numpy(synthetic.normal((B, T_obs, J, 3), seed=51)) * 0.3
    y = torch.from_numpy(synthetic.normal((B, ph, J, 3), seed=52)) * 0.3
    return y, past


def train_step_grads(m, y, past, ph):
    m.zero_grad(set_to_none=True)
    out, _, _ = m.autoencode(y, past, ph)
    m.loss(out, y).backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


MODULE_CASES = {"h36m16": (5, 7, 9), "amass21": (3, 4, 30), "release": (64, 25, 100)}
_cpu_refs = {}


def cpu_reference(case):
    """(out64, grads64, grads32) of the torch-op path on the CPU, computed once per case."""
    if case not in _cpu_refs:
        skel = "h36m16" if case == "release" else case
        B, T_obs, ph = MODULE_CASES[case]
        res = []
        for dtype in (torch.float64, torch.float32):
            m, types = make_model(skel, dtype=dtype)
            y, past = module_inputs(len(types), B, T_obs, ph)
            res.append(train_step_grads(m, y.to(dtype), past.to(dtype), ph))
        _cpu_refs[case] = (res[0][0], res[0][1], res[1][1])
    return _cpu_refs[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_module_gradients_match_float64(case, cuda):
    out64, g64, g32 = cpu_reference(case)
    skel = "h36m16" if case == "release" else case
    B, T_obs, ph = MODULE_CASES[case]
    m, types = make_model(skel, device=cuda)
    y, past = module_inputs(len(types), B, T_obs, ph)
    before = dict(training.CALLS)
    out, g = train_step_grads(m, y.to(cuda), past.to(cuda), ph)
    torch.cuda.synchronize()
    assert training.CALLS["gru_forward"] - before.get("gru_forward", 0) == 3  # past (no_grad), future, decoder
    assert training.CALLS["gru_backward"] - before.get("gru_backward", 0) == 2
    assert out.shape == (B, ph, len(types), 3)
    assert float((out.double().cpu() - out64).abs().max()) < OUT_TOL
    assert len(g) == len(g64) == 23
    report, failed = [], []
    for name in sorted(g64):
        try:
            assert_bound(f"{case} {name}", g[name], g32[name], g64[name], report)
        except AssertionError:
            failed.append(report[-1])
    assert not failed, "\n".join(failed)


# ---- routing, determinism, no_grad ------------------------------------------------------------------

def torch_autoencode(m, y, past, ph):
    """The unrolled torch-op forward (Encoder.forward / Decoder.forward through StaticGraphGRU)."""
    def encode(x):
        enc = m.encoder
        state = [(enc.initial_hidden1(x[:, 0]), None)] * enc.num_layers
        hs, _ = enc.rnn(input=x, states=state)
        return enc.activation_fn(enc.fc(enc.dropout(hs[:, -1])))

    with torch.no_grad():
        z_past = m.z_activation(encode(past))
    z = encode(y)
    dec = m.decoder
    rec_input, hidden = dec.init_recurrent_hidden(x=past[:, -2:], h=z, z=z_past)
    out = []
    for i in range(ph):
        rnn_out, hidden = dec.rnn(input=rec_input, states=hidden, t_i=i)
        out.append(dec.activation_fn(dec.fc(dec.dropout(rnn_out.squeeze(1)))))
    return torch.stack(out, dim=1)


@pytest.mark.gpu
def test_switch_off_is_bitwise_the_torch_ops(cuda):
    m, types = make_model("h36m16", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(16, 5, 7, 9))
    prev = training.set_hip_training(False)
    try:
        before = dict(training.CALLS)
        out, g = train_step_grads(m, y, past, 9)
        assert dict(training.CALLS) == before  # none of the sequence entries ran
        m.zero_grad(set_to_none=True)
        ref = torch_autoencode(m, y, past, 9)
        m.loss(ref, y).backward()
        assert torch.equal(out, ref.detach())
        for n, p in m.named_parameters():
            assert torch.equal(g[n], p.grad), n
    finally:
        training.set_hip_training(prev)


@pytest.mark.gpu
def test_switch_on_runs_the_sequence_entries_and_dropout_does_not(cuda):
    m, types = make_model("h36m16", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(16, 5, 7, 9))
    assert training.hip_training_enabled()
    before = dict(training.CALLS)
    train_step_grads(m.train(), y, past, 9)
    delta = {k: training.CALLS[k] - before.get(k, 0) for k in training.CALLS}
    assert delta == {"gru_forward": 3, "gru_backward": 2, "gx_table_forward": 1, "gx_table_backward": 1}
    # active dropout (train mode, p > 0): the torch path, which draws the masks
    m.encoder.dropout.p = m.decoder.dropout.p = 0.25
    before = dict(training.CALLS)
    train_step_grads(m.train(), y, past, 9)
    assert dict(training.CALLS) == before
    # the same p in eval mode is inactive: the sequence path again
    train_step_grads(m.eval(), y, past, 9)
    assert training.CALLS["gru_forward"] - before.get("gru_forward", 0) == 3


@pytest.mark.gpu
def test_backward_is_deterministic(cuda):
    m, types = make_model("amass21", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(21, 37, 5, 12))
    out1, g1 = train_step_grads(m, y, past, 12)
    out2, g2 = train_step_grads(m, y, past, 12)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.gpu
def test_no_grad_forward_runs_on_hip(cuda):
    m, types = make_model("h36m16", device=cuda)
    x = torch.randn((7, 9, 16, 3), generator=torch.Generator().manual_seed(5)) * 0.3  # ragged batch
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.gru_encode(sd, types, x)
    before = dict(training.CALLS)
    with torch.no_grad():
        got = m.z_activation(m(x.to(cuda)))
    torch.cuda.synchronize()
    assert training.CALLS["gru_forward"] - before.get("gru_forward", 0) == 1
    assert training.CALLS["gru_backward"] == before.get("gru_backward", 0)
    assert not got.requires_grad and float((got.cpu() - ref).abs().max()) < OUT_TOL
