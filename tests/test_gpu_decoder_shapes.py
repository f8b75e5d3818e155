"""The HIP decoder and encoder (sd_gru_decode / sd_gru_encode, `AutoEncoder.decode` /
`get_past_embedding`) against the float64 oracle beyond the H36M shape of tests/test_autoencoder.py:
every graph-linear generation the dispatch can choose from the decoder (v3 at J = 16 / 17 / 21, v2 at
N >= 512 and at other small J, v5 with its three mixing passes at J > 21), the N = 3 per-frame `fc`
launch into a strided and, at odd J, only 4-byte aligned output, the gate kernel's LDS opt-in above
64 KB, shared weights, feature sizes other than 3, zero rows of the graph matrices and saturated
gates; then the engine's workspace reuse and guard bands round `out`, `z` and the workspace.

Each case prints e32 (CPU fp32 module path vs the float64 oracle), the device error and their
ratio, and holds the device to max(200 e32, 2e-6) <= 1e-4 (decoder_cases.tolerance; the
reasoning is in that module's docstring).  tests/test_decoder_host.py checks that these inputs
tell a wrong kernel from a right one."""
import copy
import ctypes

import pytest
import torch

import decoder_cases as C
from skeletondiffusion_amd import _lib

pytestmark = pytest.mark.gpu

# (skeleton, H, L, F, B, ph): the route each is there for
DECODE_ROWS = [
    ("h36m16", 96, 96, 3, 5, 7),             # v3<16>; aligned baseline
    ("freeman17", 96, 96, 3, 5, 7),          # v3<17>; out 4-byte aligned on odd frames
    ("amass21", 96, 96, 3, 65, 5),           # v3<21>; K1 = 16 with K2 = 96; ragged row tile
    ("amass21", 192, 64, 3, 3, 4),           # N = 3 H = 576 >= 512: v2
    ("amass21", 96, 96, 3, 2, 120),          # the evaluation horizon of the J = 21 end-to-end figure
    ("mano51", 96, 96, 3, 5, 5),             # v5 exact GEMM; vector k_gl5_mix at N = 96 / 288, scalar at N = 3; gate LDS 69 KB
    ("mano52", 64, 32, 3, 9, 4),             # v5 with N = 192 / 64: the matrix-core mixing passes; fc still N = 3
    (("mod", 33, 7), 32, 16, 3, 4, 3),       # v5 at a J with no named instantiation
]
DECODE_CASES = DECODE_ROWS + [
    (("mod", 5, 3), 16, 16, 3, 3, 3),        # generic 8-node tile; smallest legal H and L
    (("mod", 64, 9), 96, 96, 3, 2, 3),       # kMaxNodes; gate LDS 88 KB
    (("none", 1), 16, 16, 3, 3, 2),          # lower edge
    (("none", 17), 96, 96, 3, 5, 4),         # num_node_types == 0 (freeman17's size)
] + [("h36m16", 32, 32, F, 3, 3) for F in (1, 6, 16)] + [  # padding at F = 1, between, F = KF (none)
    ("amass21", 32, 16, 3, B, 3) for B in (1, 63, 64, 65, 129)  # row-tile edges of every generation
] + [("amass21", 96, 96, 3, 3, 1)]           # a one-entry gx table

ENCODE_CASES = [(s, H, L, F, B, T) for (s, H, L, F, B, _) in DECODE_ROWS + [(("none", 1), 16, 16, 3, 3, 0),
                                                                            (("none", 17), 96, 96, 3, 5, 0)]
                for T in (1, 2, 9)] + [("amass21", 96, 96, 3, 3, 30)]


def _name(skel):
    return skel if isinstance(skel, str) else "-".join(str(v) for v in skel)


def _id(case):
    return "-".join([_name(case[0])] + [str(v) for v in case[1:]])


def _on(m, dev):
    """A device copy of a (shared, never modified) CPU module, with an engine of its own."""
    m = copy.deepcopy(m)
    m._engine = None
    return m.to(dev)


def _decode(m, x2, h, ph, dev):
    out = m.decode(x2.to(dev), h.to(dev), None, ph=ph)
    torch.cuda.synchronize()
    return out.cpu()


def _encode(m, x, dev):
    z = m.get_past_embedding(x.to(dev))
    torch.cuda.synchronize()
    return z.cpu()


def _check(what, got, ref, e32):
    err = C.maxdiff(got, ref)
    tol = C.tolerance(e32)
    C.report(what, e32, err, tol)
    assert torch.isfinite(got).all(), what
    assert err <= tol, (what, err, tol, e32)


@pytest.mark.parametrize("case", DECODE_CASES, ids=_id)
def test_decode_matches_oracle(case, cuda):
    skel, H, L, F, B, ph = case
    m, types, x2, h, ref, e32 = C.decode_case(*case)
    J = C.node_types(skel)[0]
    got = _decode(_on(m, cuda), x2, h, ph, cuda)
    assert got.shape == (B, ph, J, F)
    _check("decode " + _id(case), got, ref, e32)


@pytest.mark.parametrize("case", ENCODE_CASES, ids=_id)
def test_encode_matches_oracle(case, cuda):
    skel, H, L, F, B, T = case
    m, types, x, ref, e32 = C.encode_case(*case)
    J = C.node_types(skel)[0]
    got = _encode(_on(m, cuda), x, cuda)
    assert got.shape == (B, J, L)
    _check("encode " + _id(case), got, ref, e32)


# ---- special values (amass21, H = L = 32, B = 3, ph = 4) -----------------------------------------

SPECIAL = ("amass21", 32, 32, 3, 3, 4)


def _special_module():
    m, types, x2, h, _, _ = C.decode_case(*SPECIAL)
    return copy.deepcopy(m), types, x2, h


def test_zero_row_of_cell_G(cuda):
    """A zero row of the cell's G with its G_add row kept: gx_0's row is the clamp's 0 / 1e-12 = 0,
    the later rows are G_add normalised."""
    m, types, x2, h = _special_module()
    with torch.no_grad():
        m.decoder.rnn.layers[0].G[5].zero_()
        assert m.decoder.rnn.layers[0].G_add[5].abs().sum() > 0
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    _check("decode zero row 5 of rnn G", _decode(_on(m, cuda), x2, h, 4, cuda), ref, e32)
    # the encoder's table has no additive part: the row stays zero for every frame
    with torch.no_grad():
        m.encoder.rnn.layers[0].G[7].zero_()
    x = C.encode_inputs(3, 4, 21, 3, seed=77)
    zref, ez = C.encode_reference(m, types, x)
    _check("encode zero row 7 of rnn G", _encode(_on(m, cuda), x, cuda), zref, ez)


def test_zero_row_of_fc_G(cuda):
    """A zero row of fc.G: that node's output is tanh(0) = 0 exactly."""
    m, types, x2, h = _special_module()
    with torch.no_grad():
        m.decoder.fc.G[9].zero_()
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    assert (ref[:, :, 9] == 0.0).all()
    got = _decode(_on(m, cuda), x2, h, 4, cuda)
    assert (got[:, :, 9] == 0.0).all(), got[:, :, 9].abs().max().item()
    _check("decode zero row 9 of fc G", got, ref, e32)
    with torch.no_grad():
        m.decoder.initial_hidden_h.G[0].zero_()
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    _check("decode zero row 0 of initial_hidden_h G", _decode(_on(m, cuda), x2, h, 4, cuda), ref, e32)


def test_saturated_gates(cuda):
    """Frames and latents scaled by 20: the gates saturate and expf(-x) overflows to inf on one
    side; the outputs stay finite and within tolerance."""
    m, types, x2, h = _special_module()
    x2, h = x2 * 20, h * 20
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    _check("decode inputs x 20", _decode(_on(m, cuda), x2, h, 4, cuda), ref, e32)
    x = C.encode_inputs(3, 4, 21, 3, seed=78) * 20
    zref, ez = C.encode_reference(m, types, x)
    _check("encode inputs x 20", _encode(_on(m, cuda), x, cuda), zref, ez)
    # far past the overflow of expf: |W_hh hx| stays bounded, so the input side must carry it
    with torch.no_grad():
        m.decoder.rnn.layers[0].bias_ih.mul_(2000.0)  # +-200 in the gate pre-activations
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    _check("decode bias_ih x 2000", _decode(_on(m, cuda), x2, h, 4, cuda), ref, e32)


# ---- engine behaviour (amass21, H = L = 32) ------------------------------------------------------

def test_workspace_reuse_is_bitwise_stable(cuda):
    m, types, _, _, _, _ = C.decode_case(*SPECIAL)
    big_x, big_h = C.decode_inputs(129, 21, 3, 32, seed=5)
    x2, h = C.decode_inputs(2, 21, 3, 32, seed=6)
    a = _on(m, cuda)
    _decode(a, big_x, big_h, 8, cuda)
    ws = a._engine._ws
    second = _decode(a, x2, h, 3, cuda)
    assert a._engine._ws is ws  # reused while larger than needed
    fresh = _decode(_on(m, cuda), x2, h, 3, cuda)
    assert torch.equal(second, fresh)
    ref, e32 = C.decode_reference(m, types, x2, h, 3)
    _check("decode B = 2 after B = 129", second, ref, e32)


def test_encode_decode_encode_and_repeat_are_bitwise_equal(cuda):
    m, _, x2, h, _, _ = C.decode_case(*SPECIAL)
    a = _on(m, cuda)
    x = C.encode_inputs(4, 9, 21, 3, seed=7)
    z1 = _encode(a, x, cuda)
    d1 = _decode(a, x2, h, 4, cuda)
    z3 = _encode(a, x, cuda)
    d2 = _decode(a, x2, h, 4, cuda)
    assert torch.equal(z1, z3)
    assert torch.equal(d1, d2)
    assert torch.equal(_decode(a, x2, h, 4, cuda), d2)  # the same call twice in a row


def test_rows_do_not_depend_on_their_neighbours(cuda):
    m, types, _, _, _, _ = C.decode_case(*SPECIAL)
    x2, h = C.decode_inputs(65, 21, 3, 32, seed=8)
    ref, e32 = C.decode_reference(m, types, x2, h, 4)
    a = _on(m, cuda)
    whole = _decode(a, x2, h, 4, cuda)
    parts = torch.cat([_decode(a, x2[:32], h[:32], 4, cuda), _decode(a, x2[32:], h[32:], 4, cuda)])
    print(f"\n[decoder-parity] B = 65 at once vs rows 0..31 + 32..64: bitwise equal = {torch.equal(whole, parts)}, "
          f"max difference = {C.maxdiff(whole, parts):.3e}")
    _check("decode B = 65 at once", whole, ref, e32)
    _check("decode B = 65 in two parts", parts, ref, e32)
    assert C.maxdiff(whole, parts) <= C.tolerance(e32)


# ---- guard bands through the C ABI ---------------------------------------------------------------

PAD_FLOATS = 4096
SENTINEL = 0xA5


def _guarded(nbytes, dev):
    """(whole sentinel-filled byte buffer, its middle `nbytes`); the pads are PAD_FLOATS floats."""
    pad = PAD_FLOATS * 4
    whole = torch.full((pad + nbytes + pad,), SENTINEL, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 256 == 0
    return whole, whole[pad:pad + nbytes]


def _pads_intact(whole, nbytes):
    pad = PAD_FLOATS * 4
    return bool((whole[:pad] == SENTINEL).all()) and bool((whole[pad + nbytes:] == SENTINEL).all())


@pytest.mark.parametrize("skel,B,n", [("freeman17", 5, 7), ("mano51", 5, 5)])
@pytest.mark.parametrize("which", ["decode", "encode"])
def test_guard_bands(which, skel, B, n, cuda):
    """`out` / `z` in the middle of a sentinel buffer and a workspace of exactly the reported size
    inside another: nothing outside the two regions changes, and the result matches the oracle.
    (The N = 3 stores at odd J land on 4-byte aligned addresses next to the band.)"""
    L_ = _lib.lib()
    stream = torch.cuda.current_stream(cuda).cuda_stream
    if which == "decode":
        m, types, x2, h, ref, e32 = C.decode_case(skel, 96, 96, 3, B, n)
        d, keep = C.module_desc(m, "dec", cuda)
        nbytes = int(L_.sd_gru_decode_workspace_bytes(ctypes.byref(d), B, n))
    else:
        m, types, x, ref, e32 = C.encode_case(skel, 96, 96, 3, B, n)
        d, keep = C.module_desc(m, "enc", cuda)
        nbytes = int(L_.sd_gru_encode_workspace_bytes(ctypes.byref(d), B, n))
    assert nbytes > 0, L_.sd_last_error()
    out_whole, out_mid = _guarded(ref.numel() * 4, cuda)
    ws_whole, ws_mid = _guarded(nbytes, cuda)
    if which == "decode":
        xd, hd = x2.to(cuda).contiguous(), h.to(cuda).contiguous()
        _lib.check(L_.sd_gru_decode(ctypes.byref(d), xd.data_ptr(), hd.data_ptr(), B, n, out_mid.data_ptr(),
                                    ws_mid.data_ptr(), nbytes, stream))
    else:
        xd = x.to(cuda).contiguous()
        _lib.check(L_.sd_gru_encode(ctypes.byref(d), xd.data_ptr(), B, n, out_mid.data_ptr(), ws_mid.data_ptr(),
                                    nbytes, stream))
    torch.cuda.synchronize()
    assert _pads_intact(out_whole, ref.numel() * 4), "write outside the output"
    assert _pads_intact(ws_whole, nbytes), "write outside the workspace"
    got = out_mid.view(torch.float32).reshape(ref.shape).cpu()
    _check(f"{which} {skel} in guard bands", got, ref, e32)
