"""Host side of the graph-LSTM training path: the public surface, the C ABI and its
argument checks, the CPU routing, and a stand-alone program that checks the shared gate header's
backward formulas against finite differences in double under AddressSanitizer.  No GPU; the device
tests are in tests/test_gpu_lstm_train.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import lstm_cases as C
from conftest import REPO
from skeletondiffusion_amd import _lib, training

ENTRIES = ("sd_lstm_train_workspace_bytes", "sd_lstm_train_forward_workspace_bytes", "sd_lstm_train_forward",
           "sd_lstm_train_backward")


def test_public_surface():
    assert callable(training.graph_lstm) and issubclass(training.GraphLSTMFunction, torch.autograd.Function)
    assert isinstance(training.LSTM_CALLS, dict) and training.LSTM_MAX_HIDDEN == 256
    with pytest.raises(ValueError):  # no CPU path behind the explicit entry point
        training.graph_lstm(torch.zeros(1, 1, 4, 64), torch.zeros(1, 4, 16), torch.zeros(1, 4, 16), torch.eye(4),
                            torch.zeros(64, 16), None, None)


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bsize_t sd_lstm_train_workspace_bytes\(int64_t rows, int32_t T, int32_t J, int32_t H", hdr)
    assert re.search(r"\bint sd_lstm_train_forward\(const float\* a, int32_t Ta, const float\* h0, const float\* s0", hdr)
    assert re.search(r"\bint sd_lstm_train_backward\(const float\* dhs, int32_t Ta, const float\* gx", hdr)
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    assert "recurrent.py:126-167" in hdr  # the reference lines replaced
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4
    # the library still reads no environment variable
    src = open(os.path.join(REPO, "skeletondiffusion_amd", "csrc", "sd_lstm_train.hip")).read()
    assert "getenv" not in src


def host_calls():
    """(fwd, bwd) of the two entries with non-null dummy addresses: the checks return before any use."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    types16 = (ctypes.c_int64 * 16)(*([0, 1, 2, 3] * 4))

    def fwd(a=p, Ta=7, h0=p, s0=p, gx=p, Tg=1, W=p, b=p, nt=types16, n_types=4, rows=5, T=7, J=16, H=96, hs=p, s_last=p,
            P=p, gates=p, sseq=p, ws=p, ws_bytes=1 << 40, _keep=(buf, types16)):
        return L.sd_lstm_train_forward(a, Ta, h0, s0, gx, Tg, W, b, nt, n_types, rows, T, J, H, hs, s_last, P, gates, sseq,
                                       ws, ws_bytes, None)

    def bwd(dhs=p, Ta=7, gx=p, Tg=1, W=p, nt=types16, n_types=4, h0=p, s0=p, hs=p, P=p, gates=p, sseq=p, rows=5, T=7,
            J=16, H=96, ws=p, ws_bytes=1 << 40, _keep=(buf, types16)):
        return L.sd_lstm_train_backward(dhs, Ta, gx, Tg, W, nt, n_types, h0, s0, hs, P, gates, sseq, rows, T, J, H, p, p, p,
                                        p, p, p, ws, ws_bytes, None)

    return fwd, bwd


# the refusals the issue names (J = 65, H = 24, H = 272, Ta = 2 with T = 3, a node type out of range,
# a short workspace) and the rest of the argument list; each names its argument
BAD5 = (ctypes.c_int64 * 16)(*([0, 1, 2, 3] * 3 + [0, 1, 2, 4]))
NEG = (ctypes.c_int64 * 16)(*([0, -1] + [0] * 14))
REFUSALS = ((dict(J=0), b"J outside"), (dict(J=65), b"J outside"), (dict(H=0), b"H must"), (dict(H=24), b"H must"),
            (dict(H=272), b"H must"), (dict(H=-16), b"H must"), (dict(Ta=2, T=3), b"Ta must"), (dict(Ta=0), b"Ta must"),
            (dict(Tg=2), b"Tg must"), (dict(T=0), b"T must"), (dict(nt=BAD5), b"node_types[15]"),
            (dict(nt=NEG), b"node_types[1]"), (dict(nt=None), b"node_types is null"), (dict(gx=None), b"gx is null"),
            (dict(W=None), b"W_hh is null"), (dict(ws=None), b"workspace"), (dict(ws_bytes=1024), b"workspace"),
            (dict(rows=-1), b"rows"))


def check_refusals():
    L = _lib.lib()
    fwd, bwd = host_calls()
    for call, cases in ((fwd, REFUSALS + ((dict(a=None), b"a is null"), (dict(h0=None), b"h0 is null"),
                                          (dict(s0=None), b"s0 is null"), (dict(hs=None), b"hs is null"),
                                          (dict(P=None), b"all or none"))),
                        (bwd, REFUSALS + ((dict(dhs=None), b"dhs is null"), (dict(h0=None), b"h0, s0 or hs"),
                                          (dict(P=None), b"state"), (dict(sseq=None), b"state")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = L.sd_last_error()
            assert word in msg and (b"sd_lstm_train_forward" in msg or b"sd_lstm_train_backward" in msg), (kw, msg)
    need = L.sd_lstm_train_workspace_bytes(5, 7, 16, 96, 4)
    assert need > 0 and L.sd_lstm_train_workspace_bytes(5, 7, 65, 96, 4) == 0
    need_fwd = L.sd_lstm_train_forward_workspace_bytes(5, 16, 96, 4)
    assert 0 < need_fwd < need and L.sd_lstm_train_forward_workspace_bytes(5, 65, 96, 4) == 0
    assert fwd(ws_bytes=need_fwd - 1) == -1 and b"workspace" in L.sd_last_error()
    assert bwd(ws_bytes=need - 1) == -1 and b"workspace" in L.sd_last_error()
    # more rows than the dgx partials' grid takes: refused by name when dgx is asked for, not at the launch
    assert bwd(rows=262141, T=1, Ta=1) == -1 and b"too many rows for dgx" in L.sd_last_error()
    assert bwd(rows=8 * 65535 + 1, T=1, Ta=1) == -1 and b"too many rows" in L.sd_last_error()


def test_host_argument_checks():
    """Every argument is refused by name on the host, before any device call."""
    check_refusals()
    # an empty batch is no error and needs no buffer (forward); shared weights ignore node_types
    L = _lib.lib()
    assert L.sd_lstm_train_forward(None, 7, None, None, None, 1, None, None, None, 0, 0, 7, 16, 96, None, None, None, None,
                                   None, None, 0, None) == 0


def test_workspace_covers_both_directions():
    """The backward's size covers both carves and grows with every extent; the forward's does not
    depend on T."""
    L = _lib.lib()
    base = L.sd_lstm_train_workspace_bytes(5, 7, 16, 96, 4)
    fwd = L.sd_lstm_train_forward_workspace_bytes(5, 16, 96, 4)
    B, T, J, H = 5, 7, 16, 96
    assert base >= 4 * (2 * B * T * J * 4 * H + B * T * J * H + 2 * B * J * H)   # dQ, dP, h_{t-1}, the two carries
    assert base >= fwd >= 4 * (4 * 4 * H * H + B * J * 4 * H + 2 * B * J * H)    # W^T, P_t, the two s slabs
    assert fwd < 4 * (4 * 4 * H * H + B * J * 4 * H + 2 * B * J * H) + 4 * 256     # and no more (256-B rounding)
    assert L.sd_lstm_train_workspace_bytes(5, 1, 16, 96, 4) >= fwd
    for bigger in ((6, 7, 16, 96), (5, 8, 16, 96), (5, 7, 17, 96), (5, 7, 16, 112)):
        assert L.sd_lstm_train_workspace_bytes(*bigger, 4) > base


@pytest.mark.parametrize("arch", list(C.ARCHS))
def test_cpu_autoencode_is_the_torch_path_whatever_the_switch(arch):
    m = C.make_model(arch)
    past, _, y = C.fixture_inputs()
    past, y = past[:, :5], y[:, :4]
    ref = {}
    before = (dict(training.CALLS), dict(training.LSTM_CALLS))
    for flag in (True, False):
        prev = training.set_hip_training(flag)
        try:
            out, _, _, _, grads = C.train_step_grads(m, y, past, 4)
        finally:
            training.set_hip_training(prev)
        if not ref:
            ref = dict(out=out, grads=grads)
            continue
        assert torch.equal(out, ref["out"])
        for n, g in grads.items():
            assert (g is None and ref["grads"][n] is None) or torch.equal(g, ref["grads"][n]), n
    assert (dict(training.CALLS), dict(training.LSTM_CALLS)) == before


def test_gate_backward_matches_finite_differences_under_asan(tmp_path):
    """tests/host/lstm_train_emulation.cpp restates the core in double over csrc/sd_lstm_gates.h (the
    kernels' gate math and index arithmetic) at the smallest GPU-test shapes, every Ta / Tg
    combination, repeated types, with and without bias, and compares every gradient with central
    finite differences; AddressSanitizer + UBSan."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lstm_train_emulation")
    src = os.path.join(REPO, "tests", "host", "lstm_train_emulation.cpp")
    # the sanitizer runtime is linked statically (g++ -static-libasan; clang's default), so the program
    # needs nothing preloaded and does not mind what its environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "lstm train emulation ok" in r.stdout
