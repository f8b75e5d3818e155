"""Training the graph-LSTM autoencoder on HIP: the sequence core
(`training.graph_lstm`) against its float64 restatement (tests/lstm_cases.py:core_ref), the whole
module's autoencode + loss + backward against float64 on the CPU, the reference's fixture
(tests/golden/lstm.npz) on the device, and the invariants of the entry points.

Yardsticks, those of tests/test_gpu_gru_train.py: forward max|hs - hs64| < 1e-5; per gradient tensor
err = max|g - g64| / max|g64| (no absolute floor) with the bound err_hip <= 8 x err_torch32,
err_torch32 being the same torch-op path in float32 on the CPU for the same tensor and inputs,
computed here; a tensor whose float64 gradient is identically zero must be exactly zero; decoded
frames within 1e-4 of float64."""
import pytest
import torch

import lstm_cases as C
from skeletondiffusion_amd import training
from test_lstm_train_host import check_refusals

FACTOR = 8.0
FWD_TOL = 1e-5   # forward of the core
OUT_TOL = 1e-4   # decoded frames / latents of the module


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


def maxdiff(a, ref):
    return float((a.detach().double().cpu() - torch.as_tensor(ref).double()).abs().max())


# ---- the core against its float64 restatement -------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("J,H,B,T,Ta,Tg,typed,bias", C.CORE_CASES)
def test_core_matches_float64(J, H, B, T, Ta, Tg, typed, bias, cuda):
    inp = C.core_inputs(J, H, B, T, Ta, Tg, typed, bias, seed=J * 1000 + B)
    hs64, s64, g64 = C.run_core(inp, T, dtype=torch.float64)
    _, _, g32 = C.run_core(inp, T, dtype=torch.float32)
    hs, s_last, g = C.run_core(inp, T, dtype=torch.float32, device=cuda, hip=True)
    torch.cuda.synchronize()
    assert hs.shape == (B, T, J, H) and s_last.shape == (B, J, H)
    print(f"core {(J, H, B, T, Ta, Tg)} forward: hs {maxdiff(hs, hs64):.3e} s_last {maxdiff(s_last, s64):.3e}")
    assert maxdiff(hs, hs64) < FWD_TOL and maxdiff(s_last, s64) < FWD_TOL
    report, failed = [], []
    for k in g64:
        assert g[k].shape == inp[k].shape
        try:
            assert_bound(f"core {(J, H, B, T, Ta, Tg)} d{k}", g[k], g32[k], g64[k], report)
        except AssertionError:
            failed.append(report[-1])
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
def test_core_empty_batch(cuda):
    inp = C.core_inputs(16, 96, 0, 3, 3, 1, True, True, seed=1)
    hs, s_last, g = C.run_core(inp, 3, dtype=torch.float32, device=cuda, hip=True)
    torch.cuda.synchronize()
    assert hs.shape == (0, 3, 16, 96) and s_last.shape == (0, 16, 96)
    for k in ("gx", "W", "b"):
        assert g[k].shape == inp[k].shape and float(g[k].abs().max()) == 0.0
    assert g["a"].shape == (0, 3, 16, 384) and g["h0"].shape == (0, 16, 96) and g["s0"].shape == (0, 16, 96)


@pytest.mark.gpu
def test_core_backward_twice_and_no_grad_forward_are_bitwise(cuda):
    inp = C.core_inputs(17, 32, 37, 3, 1, 3, True, True, seed=5)
    hs1, s1, g1 = C.run_core(inp, 3, dtype=torch.float32, device=cuda, hip=True)
    hs2, s2, g2 = C.run_core(inp, 3, dtype=torch.float32, device=cuda, hip=True)
    x = {k: inp[k].to(cuda) for k in C.CORE_NAMES}
    before = dict(training.LSTM_CALLS)
    with torch.no_grad():
        hs3, s3 = training.graph_lstm(x["a"], x["h0"], x["s0"], x["gx"], x["W"], x["b"], inp["types"], steps=3)
    torch.cuda.synchronize()
    assert training.LSTM_CALLS["lstm_forward"] - before.get("lstm_forward", 0) == 1
    assert not hs3.requires_grad and not s3.requires_grad
    assert torch.equal(hs1, hs2) and torch.equal(s1, s2) and torch.equal(hs1, hs3) and torch.equal(s1, s3)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.gpu
def test_s_last_is_not_differentiable(cuda):
    inp = C.core_inputs(16, 16, 2, 2, 2, 1, False, True, seed=3)
    x = {k: inp[k].to(cuda).requires_grad_(True) for k in C.CORE_NAMES}
    hs, s_last = training.graph_lstm(x["a"], x["h0"], x["s0"], x["gx"], x["W"], x["b"], None, steps=2)
    assert hs.requires_grad and not s_last.requires_grad


@pytest.mark.gpu
def test_host_refusals_launch_nothing(cuda):
    """J = 65, H = 24, H = 272, Ta = 2 with T = 3, a node type out of range, a short workspace (and the
    rest of tests/test_lstm_train_host.py's list) return SD_E_INVALID naming the argument, from dummy
    host addresses no kernel could have read; the device is still healthy afterwards."""
    torch.zeros(1, device=cuda)
    check_refusals()
    torch.cuda.synchronize()
    inp = C.core_inputs(16, 96, 2, 3, 3, 1, True, True, seed=2)
    x = {k: inp[k].to(cuda) for k in C.CORE_NAMES}
    with pytest.raises(Exception) as e:  # 8 weight types, every node asks for the tenth
        training.graph_lstm(x["a"], x["h0"], x["s0"], x["gx"], x["W"], x["b"], torch.full((16,), 9), steps=3)
    assert "node_types[0]" in str(e.value)
    with pytest.raises(Exception) as e:  # Ta = 2 with T = 3
        training.graph_lstm(x["a"][:, :2], x["h0"], x["s0"], x["gx"], x["W"], x["b"], inp["types"], steps=3)
    assert "Ta must" in str(e.value)
    torch.cuda.synchronize()


# ---- the whole module ---------------------------------------------------------------------------------

def module_inputs(J, B, T_obs, ph):
    from skeletondiffusion_amd import synthetic

    past = torch.from_numpy(synthetic.normal((B, T_obs, J, 3), seed=51)) * 0.3
    y = torch.from_numpy(synthetic.normal((B, ph, J, 3), seed=52)) * 0.3
    return y, past


MODULE_CASES = {"ll-h36m16": ("ll", "h36m16", (5, 7, 9)), "lg-h36m16": ("lg", "h36m16", (5, 7, 9)),
                "gl-h36m16": ("gl", "h36m16", (5, 7, 9)), "ll-amass21": ("ll", "amass21", (3, 4, 30))}
_cpu_refs = {}


def cpu_reference(case):
    """(out64, grads64, grads32) of the torch-op path on the CPU, computed once per case."""
    if case not in _cpu_refs:
        arch, skel, (B, T_obs, ph) = MODULE_CASES[case]
        res = []
        for dtype in (torch.float64, torch.float32):
            m = C.make_model(arch, skel, dtype=dtype)
            y, past = module_inputs(m.encoder.rnn.layers[0].num_nodes, B, T_obs, ph)
            r = C.train_step_grads(m, y.to(dtype), past.to(dtype), ph)
            res.append((r[0], r[4]))
        _cpu_refs[case] = (res[0][0], res[0][1], res[1][1])
    return _cpu_refs[case]


def lstm_sides(arch):
    return sum(a == C.LSTM for a in C.ARCHS[arch])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_module_gradients_match_float64(case, cuda):
    out64, g64, g32 = cpu_reference(case)
    arch, skel, (B, T_obs, ph) = MODULE_CASES[case]
    m = C.make_model(arch, skel, device=cuda)
    J = m.encoder.rnn.layers[0].num_nodes
    y, past = module_inputs(J, B, T_obs, ph)
    before = dict(training.LSTM_CALLS)
    out, _, _, _, g = C.train_step_grads(m, y.to(cuda), past.to(cuda), ph)
    torch.cuda.synchronize()
    enc_lstm, dec_lstm = (a == C.LSTM for a in C.ARCHS[arch])
    # an LSTM encoder runs twice (past under no_grad, future), an LSTM decoder once
    assert training.LSTM_CALLS["lstm_forward"] - before.get("lstm_forward", 0) == 2 * enc_lstm + dec_lstm
    assert training.LSTM_CALLS["lstm_backward"] - before.get("lstm_backward", 0) == enc_lstm + dec_lstm
    assert out.shape == (B, ph, J, 3)
    print(f"{case} decoded frames: {maxdiff(out, out64):.3e}")
    assert maxdiff(out, out64) < OUT_TOL
    assert sorted(g) == sorted(g64)
    report, failed = [], []
    for name in sorted(g64):
        if g64[name] is None:
            assert name.endswith("bias_ih") and "rnn" in name and g[name] is None, name
            continue
        try:
            assert_bound(f"{case} {name}", g[name], g32[name], g64[name], report)
        except AssertionError:
            failed.append(report[-1])
    assert sum(v is None for v in g.values()) == lstm_sides(arch)
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ll", "lls", "lg", "gl"])
def test_fixture_embedding_and_decode_on_the_device(name, cuda):
    """get_past_embedding and decode of the reference's fixture, the scaled set included: an LSTM side
    through the HIP sequence forward under no_grad, a GRU side through the GRU engine."""
    z = C.load_golden()
    arch, scale = ("ll", C.SCALE) if name == "lls" else (name, 1.0)
    m = C.make_model(arch, device=cuda, scale=scale)
    past, lat, _ = (v.to(cuda) for v in C.fixture_inputs())
    before = dict(training.LSTM_CALLS)
    zp = m.get_past_embedding(past)
    out = m.decode(past.repeat_interleave(4, 0), lat, None, ph=C.PH)
    torch.cuda.synchronize()
    assert training.LSTM_CALLS["lstm_forward"] - before.get("lstm_forward", 0) == lstm_sides(arch)
    assert training.LSTM_CALLS["lstm_backward"] == before.get("lstm_backward", 0)
    assert not zp.requires_grad and not out.requires_grad
    print(f"{name}: z_past {maxdiff(zp, z[f'{name}_z_past']):.3e} decode {maxdiff(out, z[f'{name}_dec']):.3e}")
    assert maxdiff(zp, z[f"{name}_z_past"]) < OUT_TOL
    assert maxdiff(out, z[f"{name}_dec"]) < OUT_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("hip_only", [False, True])
def test_forwards_without_grad_keep_no_state(hip_only, cuda):
    """get_past_embedding, decode, autoencode's z_past and a whole no_grad autoencode of a module with
    default (requires_grad) parameters keep none of the backward's state, with and without
    hip_forward_only(): the counter of kept forwards does not move, and the peak allocation of a
    decode stays below the size of that state (P and gates 4H each, s_t H floats per row, step, node),
    where the outputs, the projections and the forward-only workspace are a small fraction of it."""
    import contextlib

    m = C.make_model("ll", device=cuda)
    assert all(p.requires_grad for p in m.parameters())
    past, lat, y = (v.to(cuda) for v in C.fixture_inputs())
    rows, ph, J, H = 192, 40, 16, 96
    past_r, lat_r = past.repeat(rows // 3, 1, 1, 1), lat.repeat(rows // 12, 1, 1)
    scope = training.hip_forward_only if hip_only else contextlib.nullcontext
    before = dict(training.STATE_KEPT), dict(training.LSTM_CALLS)
    with scope():
        m.get_past_embedding(past)
        m.decode(past_r, lat_r, None, ph=4)   # warm: library load, cached node types and identity
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(cuda)
        base = torch.cuda.memory_allocated(cuda)
        out = m.decode(past_r, lat_r, None, ph=ph)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(cuda) - base
        with torch.no_grad():
            m.autoencode(y, past, C.PH)
    assert out.shape == (rows, ph, J, 3)
    assert training.LSTM_CALLS["lstm_forward"] - before[1].get("lstm_forward", 0) == 6
    assert training.STATE_KEPT["lstm"] == before[0].get("lstm", 0)
    state_bytes = rows * ph * J * 9 * H * 4
    print(f"decode {rows} x {ph}: peak {peak / 2**20:.1f} MiB, kept state would be {state_bytes / 2**20:.1f} MiB")
    assert peak < state_bytes / 2
    # under grad the z_past encode still keeps nothing; the future's encode and the decode do
    m.autoencode(y, past, C.PH)
    assert training.STATE_KEPT["lstm"] - before[0].get("lstm", 0) == 2


# ---- routing, determinism -----------------------------------------------------------------------------

def torch_autoencode(m, y, past, ph):
    """The unrolled torch-op forward, cell by cell, whatever the architectures."""
    def encode(x):
        enc = m.encoder
        init = (enc.initial_hidden1(x[:, 0]),) + ((enc.initial_hidden_c(x[:, 0]),) if hasattr(enc, "initial_hidden_c") else ())
        hs, _ = enc.rnn(input=x, states=[init + (None,)] * enc.num_layers)
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
    m = C.make_model("ll", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(16, 5, 7, 9))
    prev = training.set_hip_training(False)
    try:
        before = (dict(training.CALLS), dict(training.LSTM_CALLS))
        out, _, _, _, g = C.train_step_grads(m, y, past, 9)
        assert (dict(training.CALLS), dict(training.LSTM_CALLS)) == before  # none of the sequence entries ran
        m.zero_grad(set_to_none=True)
        ref = torch_autoencode(m, y, past, 9)
        m.loss(ref, y).backward()
        assert torch.equal(out, ref.detach())
        for n, p in m.named_parameters():
            assert (g[n] is None and p.grad is None) or torch.equal(g[n], p.grad), n
    finally:
        training.set_hip_training(prev)


@pytest.mark.gpu
def test_switch_on_runs_the_sequence_entries_and_dropout_does_not(cuda):
    m = C.make_model("ll", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(16, 5, 7, 9))
    assert training.hip_training_enabled()
    before = dict(training.LSTM_CALLS)
    C.train_step_grads(m.train(), y, past, 9)
    assert {k: training.LSTM_CALLS[k] - before.get(k, 0) for k in training.LSTM_CALLS} == \
        {"lstm_forward": 3, "lstm_backward": 2}
    # active dropout (train mode, p > 0): the torch path, which draws the masks
    m.encoder.dropout.p = m.decoder.dropout.p = 0.25
    before = dict(training.LSTM_CALLS)
    C.train_step_grads(m.train(), y, past, 9)
    assert dict(training.LSTM_CALLS) == before
    # the same p in eval mode is inactive: the sequence path again
    C.train_step_grads(m.eval(), y, past, 9)
    assert training.LSTM_CALLS["lstm_forward"] - before.get("lstm_forward", 0) == 3


@pytest.mark.gpu
def test_module_backward_is_deterministic(cuda):
    m = C.make_model("ll", "amass21", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(21, 37, 5, 12))
    out1, _, _, _, g1 = C.train_step_grads(m, y, past, 12)
    out2, _, _, _, g2 = C.train_step_grads(m, y, past, 12)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    for n in g1:
        assert (g1[n] is None and g2[n] is None) or torch.equal(g1[n], g2[n]), n


@pytest.mark.gpu
def test_no_grad_module_forward_equals_the_grad_forward(cuda):
    """Under hip_forward_only() every gate passes without grad, so the very same kernels run: bitwise
    (z_past apart: autoencode always computes it under a plain no_grad).  Plain no_grad normalises the
    mixing matrices with torch ops instead: within the output tolerance."""
    m = C.make_model("ll", device=cuda)
    y, past = (v.to(cuda) for v in module_inputs(16, 7, 9, 5))   # ragged batch
    out, z_past, z = m.autoencode(y, past, 5)
    with torch.no_grad(), training.hip_forward_only():
        out2, z_past2, z2 = m.autoencode(y, past, 5)
    with torch.no_grad():
        out3, _, _ = m.autoencode(y, past, 5)
    torch.cuda.synchronize()
    assert out.requires_grad and not out2.requires_grad and not out3.requires_grad
    assert torch.equal(out.detach(), out2) and torch.equal(z.detach(), z2)
    assert maxdiff(z_past2, z_past.cpu()) < OUT_TOL
    assert maxdiff(out3, out.detach().cpu()) < OUT_TOL
