"""Host side of the graph-GRU training path: the public surface, the C ABI and its
argument checks, the CPU routing, and a stand-alone program that checks the shared gate header's
backward formulas and the gx-table backward against finite differences in double under
AddressSanitizer.  No GPU; the device tests are in tests/test_gpu_gru_train.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import REPO
from skeletondiffusion_amd import _lib, synthetic, training
from skeletondiffusion_amd.skeletons import skeleton

ENTRIES = ("sd_gru_train_workspace_bytes", "sd_gru_train_forward", "sd_gru_train_backward", "sd_gx_table_forward",
           "sd_gx_table_backward")


def test_public_surface():
    assert callable(training.graph_gru) and callable(training.gx_table)
    assert isinstance(training.CALLS, dict)
    with pytest.raises(ValueError):  # no CPU path behind the explicit entry points
        training.graph_gru(torch.zeros(1, 1, 4, 48), torch.zeros(1, 4, 16), torch.eye(4), torch.zeros(48, 16), None, None)
    with pytest.raises(ValueError):
        training.gx_table(torch.eye(4), None, 3)


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bsize_t sd_gru_train_workspace_bytes\(int64_t rows, int32_t T, int32_t J, int32_t H", hdr)
    assert re.search(r"\bint sd_gru_train_forward\(const float\* a, int32_t Ta, const float\* h0", hdr)
    assert re.search(r"\bint sd_gru_train_backward\(const float\* dhs, const float\* a, int32_t Ta", hdr)
    assert re.search(r"\bint sd_gx_table_forward\(const float\* G, const float\* G_add, int32_t J, int32_t T", hdr)
    assert re.search(r"\bint sd_gx_table_backward\(const float\* G, const float\* G_add, const float\* gxt", hdr)
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    assert "recurrent.py:321-366" in hdr and "trainer.py:79-96" in hdr  # the reference lines replaced
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4


def test_host_argument_checks():
    """Every argument is refused by name on the host, before any device call."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)
    types16 = (ctypes.c_int64 * 16)(*([0, 1, 2, 3] * 4))

    def fwd(a=p, Ta=7, h0=p, gx=p, Tg=1, W=p, b=p, nt=types16, n_types=4, rows=5, T=7, J=16, H=96, hs=p, hprev=p, c=p,
            gates=p, ws=p, ws_bytes=1 << 40):
        return L.sd_gru_train_forward(a, Ta, h0, gx, Tg, W, b, nt, n_types, rows, T, J, H, hs, hprev, c, gates, ws, ws_bytes,
                                      None)

    def bwd(dhs=p, a=p, Ta=7, gx=p, Tg=1, W=p, nt=types16, n_types=4, hprev=p, c=p, gates=p, rows=5, T=7, J=16, H=96,
            ws=p, ws_bytes=1 << 40):
        return L.sd_gru_train_backward(dhs, a, Ta, gx, Tg, W, nt, n_types, hprev, c, gates, rows, T, J, H, p, p, p, p, p, ws,
                                       ws_bytes, None)

    bad5 = (ctypes.c_int64 * 16)(*([0, 1, 2, 3] * 3 + [0, 1, 2, 4]))
    neg = (ctypes.c_int64 * 16)(*([0, -1] + [0] * 14))
    common = ((dict(J=0), b"J outside"), (dict(J=65), b"J outside"), (dict(H=0), b"H must"), (dict(H=24), b"H must"),
              (dict(H=-16), b"H must"), (dict(Ta=3), b"Ta must"), (dict(Ta=0), b"Ta must"), (dict(Tg=2), b"Tg must"),
              (dict(T=0), b"T must"), (dict(nt=bad5), b"node_types[15]"), (dict(nt=neg), b"node_types[1]"),
              (dict(nt=None), b"node_types is null"), (dict(a=None), b"a is null"), (dict(gx=None), b"gx is null"),
              (dict(W=None), b"W_hh is null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=1024), b"workspace"),
              (dict(rows=-1), b"rows"))
    for call, cases in ((fwd, common + ((dict(h0=None), b"h0 is null"), (dict(hs=None), b"hs is null"),
                                         (dict(c=None), b"all or none"))),
                        (bwd, common + ((dict(dhs=None), b"dhs is null"), (dict(hprev=None), b"state"),
                                         (dict(gates=None), b"state")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())
    # an empty batch is no error and needs no buffer (forward); shared weights ignore node_types
    assert L.sd_gru_train_forward(None, 7, None, None, 1, None, None, None, 0, 0, 7, 16, 96, None, None, None, None, None, 0,
                                  None) == 0
    need = L.sd_gru_train_workspace_bytes(5, 7, 16, 96, 4)
    assert need > 0 and L.sd_gru_train_workspace_bytes(5, 7, 65, 96, 4) == 0
    assert fwd(ws_bytes=need - 1) == -1 and b"workspace" in L.sd_last_error()

    def tab(G=p, J=16, T=3, out=p):
        return L.sd_gx_table_forward(G, p, J, T, 1, 1e-12, out, None)

    def tab_b(G=p, gxt=p, dgxt=p, J=16, T=3, dG=p):
        return L.sd_gx_table_backward(G, p, gxt, dgxt, J, T, 1, 1e-12, dG, p, None)

    for call, cases in ((tab, ((dict(J=0), b"J outside"), (dict(J=65), b"J outside"), (dict(T=0), b"T must"),
                               (dict(G=None), b"G is null"), (dict(out=None), b"gxt is null"))),
                        (tab_b, ((dict(J=65), b"J outside"), (dict(T=0), b"T must"), (dict(G=None), b"G is null"),
                                 (dict(gxt=None), b"gxt is null"), (dict(dgxt=None), b"dgxt is null"),
                                 (dict(dG=None), b"dG is null")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())


def _model():
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    _, _, _, types = skeleton("h36m16")
    m = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=16, encoder_hidden_size=96, decoder_hidden_size=96,
                    latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                    recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU", if_consider_hip=False)
    synthetic.fill_module_(m, 4321)
    return m


def _unrolled(m, y, past, ph):
    """The torch-op forward, cell by cell (Encoder.forward / Decoder.forward through StaticGraphGRU)."""
    def encode(x):
        enc = m.encoder
        hs, _ = enc.rnn(input=x, states=[(enc.initial_hidden1(x[:, 0]), None)])
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


def test_cpu_autoencode_is_the_torch_path_whatever_the_switch():
    m = _model()
    past = torch.from_numpy(synthetic.normal((3, 5, 16, 3), seed=51)) * 0.3
    y = torch.from_numpy(synthetic.normal((3, 4, 16, 3), seed=52)) * 0.3
    ref = _unrolled(m, y, past, 4)
    m.loss(ref, y).backward()
    gref = {n: p.grad.clone() for n, p in m.named_parameters()}
    before = dict(training.CALLS)
    for flag in (True, False):
        prev = training.set_hip_training(flag)
        try:
            m.zero_grad(set_to_none=True)
            out, _, _ = m.autoencode(y, past, 4)
            m.loss(out, y).backward()
        finally:
            training.set_hip_training(prev)
        assert torch.equal(out, ref)
        for n, p in m.named_parameters():
            assert torch.equal(p.grad, gref[n]), n
    assert dict(training.CALLS) == before


def test_gate_and_table_backward_match_finite_differences_under_asan(tmp_path):
    """tests/host/gru_train_emulation.cpp restates the core in double over csrc/sd_gru_gates.h (the
    kernels' gate math and index arithmetic) at the smallest GPU-test shapes and compares every
    gradient, and the gx table's, with central finite differences; AddressSanitizer + UBSan."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gru_train_emulation")
    src = os.path.join(REPO, "tests", "host", "gru_train_emulation.cpp")
    # the sanitizer runtime is linked statically (g++ -static-libasan; clang's default), so the program
    # needs nothing preloaded and does not mind what its environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "gru train emulation ok" in r.stdout
