"""Graph-LSTM autoencoder (StaticGraphLSTM encoders / decoders) on the CPU against
the reference's own outputs (tests/golden/lstm.npz, gen_golden_lstm.py): state-dict keys, the torch-op
path in float32 (1e-6) and float64 (1e-10), float64 gradients (1e-9 relative), the reference's quirks
(`bias_ih` unused, `init_weights` copying block 0), and the unchanged GRU module.  The fixture holds
the reference's float64 outputs; its float32 outputs were within 1.4e-7 of them when it was written,
so the float32 path is held to 1e-6 against float64.  No GPU; the device tests are in
tests/test_gpu_lstm_train.py."""
import numpy as np
import pytest
import torch

import lstm_cases as C
from conftest import golden

TOL = {torch.float32: 1e-6, torch.float64: 1e-10}
GRAD_RTOL = 1e-9
SETS = {"ll": ("ll", 1.0), "lg": ("lg", 1.0), "gl": ("gl", 1.0), "lls": ("ll", C.SCALE)}


def maxdiff(a, ref):
    return float((a.detach().double() - torch.from_numpy(np.asarray(ref))).abs().max())


@pytest.mark.parametrize("arch", list(C.ARCHS))
def test_state_dict_keys_match_reference(arch):
    z = C.load_golden()
    m = C.make_model(arch)
    keys = sorted(m.state_dict().keys())
    assert keys == list(z[f"{arch}_keys"]) and len(keys) == C.N_KEYS[arch]
    enc_lstm, dec_lstm = (a == C.LSTM for a in C.ARCHS[arch])
    assert hasattr(m.encoder, "initial_hidden_c") == enc_lstm and hasattr(m.decoder, "initial_hidden_c") == dec_lstm


@pytest.mark.parametrize("arch", list(C.ARCHS))
def test_state_dict_round_trips_strictly(arch):
    src = C.make_model(arch)
    dst = C.make_model(arch)
    with torch.no_grad():
        for p in dst.parameters():
            p.zero_()
    dst.load_state_dict(src.state_dict(), strict=True)
    for (n, a), (_, b) in zip(sorted(src.state_dict().items()), sorted(dst.state_dict().items())):
        assert torch.equal(a, b), n
    with pytest.raises(RuntimeError):  # an LSTM checkpoint does not fit a GRU module, strictly
        from test_autoencoder import _model
        _model()[0].load_state_dict(src.state_dict(), strict=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", list(SETS))
def test_torch_path_matches_reference(name, dtype):
    z = C.load_golden()
    arch, scale = SETS[name]
    m = C.make_model(arch, dtype=dtype, scale=scale)
    past, lat, y = (v.to(dtype) for v in C.fixture_inputs())
    tol = TOL[dtype]
    assert maxdiff(C.encode(m, past), z[f"{name}_z_past"]) < tol
    assert maxdiff(C.decode(m, past, lat), z[f"{name}_dec"]) < tol
    out, z_past, zz = m.autoencode(y, past, ph=C.PH)
    assert out.shape == (3, C.PH, 16, 3)
    assert maxdiff(out, z[f"{name}_ae_out"]) < tol
    assert maxdiff(z_past, z[f"{name}_z_past"]) < tol
    assert maxdiff(zz, z[f"{name}_ae_z"]) < tol
    assert maxdiff(m.loss(out, y), z[f"{name}_ae_loss"]) < tol


@pytest.mark.parametrize("name", ["ll", "lls"])
def test_gradients_match_reference_float64(name):
    z = C.load_golden()
    arch, scale = SETS[name]
    m = C.make_model(arch, dtype=torch.float64, scale=scale)
    past, _, y = (v.double() for v in C.fixture_inputs())
    grads = C.train_step_grads(m, y, past, C.PH)[4]
    names = list(z[f"{name}_gnames"])
    assert sorted(n for n, g in grads.items() if g is not None) == names
    assert sorted(n for n, g in grads.items() if g is None) == list(z[f"{name}_gnone"])
    for k, n in enumerate(names):
        smp, s, nrm = C.grad_sample(grads[n])
        ref = torch.from_numpy(z[f"{name}_g/{n}"])
        ref_sum, ref_nrm = float(z[f"{name}_gsum"][k]), float(z[f"{name}_gnorm"][k])
        assert ref_nrm > 0.0, n
        assert smp.shape == ref.shape
        assert float((smp - ref).abs().max()) <= GRAD_RTOL * float(ref.abs().max()), n
        assert abs(float(nrm) - ref_nrm) <= GRAD_RTOL * ref_nrm, n
        assert abs(float(s) - ref_sum) <= GRAD_RTOL * max(abs(ref_sum), ref_nrm), n


def test_scaled_set_leaves_the_linear_range():
    z = C.load_golden()
    assert float(z["scale"]) == C.SCALE
    assert float(z["lls_qmax"]) >= 2.0 and float(z["lls_decmax"]) >= 0.3
    assert float(np.abs(z["lls_dec"]).max()) == float(z["lls_decmax"])


def test_bias_ih_is_a_key_without_a_gradient():
    m = C.make_model("ll")
    past, _, y = C.fixture_inputs()
    grads = C.train_step_grads(m, y, past, C.PH)[4]
    for side in ("encoder", "decoder"):
        assert f"{side}.rnn.layers.0.bias_ih" in m.state_dict()
        assert grads[f"{side}.rnn.layers.0.bias_ih"] is None
        assert grads[f"{side}.rnn.layers.0.bias_hh"] is not None
    assert m.encoder.rnn.layers[0].bias_ih.grad is None


def test_init_weights_copies_the_first_block():
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder, StaticGraphLSTMCell
    from skeletondiffusion_amd.skeletons import skeleton

    _, _, _, types = skeleton("h36m16")
    torch.manual_seed(0)
    m = AutoEncoder(node_types=torch.from_numpy(types), **C.ae_kwargs(16, C.LSTM, C.LSTM))
    for cell in (m.encoder.rnn.layers[0], m.decoder.rnn.layers[0]):
        assert cell.weight_hh.dim() == 3 and cell.weight_hh.shape[0] > 1
        for w in (cell.weight_hh, cell.weight_ih):
            assert bool((w[1:] == w[0]).all())
        assert not bool((cell.bias_hh[1:] == cell.bias_hh[0]).all())
        assert float(cell.weight_hh.detach().abs().max()) <= 1.0 / 96 ** 0.5
    # shared weights: a 2-D weight_hh has its rows copied (weight.data[1:] = weight.data[0]), weight_ih not
    cell = StaticGraphLSTMCell(3, 16, num_nodes=5)
    assert cell.weight_hh.shape == (64, 16) and bool((cell.weight_hh[1:] == cell.weight_hh[0]).all())
    assert not bool((cell.weight_ih[1:] == cell.weight_ih[0]).all())


def test_gru_module_is_unchanged():
    """A GRU/GRU module: the keys and outputs of tests/golden/decoder.npz, and 2-tuples of state."""
    from test_autoencoder import _inputs, _model

    z = golden("decoder")
    m, _ = _model()
    assert sorted(m.state_dict().keys()) == list(z["keys"]) and len(z["keys"]) == 27
    assert not hasattr(m.encoder, "initial_hidden_c") and not hasattr(m.decoder, "initial_hidden_c")
    past, lat = _inputs()
    with torch.no_grad():
        h, state = m.encoder(past)
        out, _ = m.decoder(x=past.repeat_interleave(4, 0)[:, -2:], h=lat, z=None, ph=120)
    assert len(state[0]) == 2
    assert maxdiff(m.z_activation(h), z["z_past"]) < 1e-5 and maxdiff(out, z["out"]) < 1e-5


def test_unknown_arch_is_refused():
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    with pytest.raises(NotImplementedError):
        AutoEncoder(**C.ae_kwargs(16, "StaticGraphRNN", C.GRU))


def test_lstm_states_are_triples():
    m = C.make_model("ll")
    past, _, _ = C.fixture_inputs()
    with torch.no_grad():
        _, state = m.encoder(past[:, :4])
    h, s, gx = state[0]
    assert h.shape == s.shape == (3, 16, 96) and gx.shape == (16, 16)


@pytest.mark.parametrize("name", ["ll", "lls", "lg", "gl"])
def test_embedding_and_decode_run_on_the_cpu(name):
    """AutoEncoder.get_past_embedding / decode of a module whose encoder / decoder is an LSTM run that
    module's forward under no_grad (torch ops on the CPU); a GRU side still asks for the HIP engine."""
    from skeletondiffusion_amd._lib import SkelDiffError

    z = C.load_golden()
    arch, scale = SETS[name]
    m = C.make_model(arch, scale=scale)
    past, lat, _ = C.fixture_inputs()
    enc_lstm, dec_lstm = (a == C.LSTM for a in C.ARCHS[arch])
    if enc_lstm:
        zp = m.get_past_embedding(past)
        assert not zp.requires_grad and maxdiff(zp, z[f"{name}_z_past"]) < 1e-6
    else:
        with pytest.raises(SkelDiffError):
            m.get_past_embedding(past)
    if dec_lstm:
        out = m.decode(past.repeat_interleave(4, 0), lat, None, ph=C.PH)
        assert not out.requires_grad and maxdiff(out, z[f"{name}_dec"]) < 1e-6
    else:
        with pytest.raises(SkelDiffError):
            m.decode(past.repeat_interleave(4, 0), lat, None, ph=C.PH)
