"""Host side of the HIP encoder / decoder parity tests (tests/test_gpu_decoder_shapes.py):
the oracle's shared-weight path, a guard on the fixtures (every deliberate error a kernel could
make moves the reference by at least 10 times the tolerance the device is held to), and the
argument validation of sd_gru_decode / sd_gru_encode, which runs before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import decoder_cases as C
import oracle as O
from skeletondiffusion_amd import _lib

SD_OK, SD_E_INVALID = 0, -1


def test_oracle_untyped_matches_module():
    """node_types=None (2-D weights, 1-D biases shared by every node) at J = 17: the float64 oracle
    equals the CPU torch module path within 1e-6, decoder and encoder."""
    m, types = C.build(("none", 17), 96, 96)
    assert types is None and m.decoder.fc.weight.dim() == 2 and m.decoder.rnn.layers[0].bias_hh.dim() == 1
    x2, h = C.decode_inputs(5, 17, 3, 96, seed=3)
    ref, e32 = C.decode_reference(m, None, x2, h, 31)
    assert ref.shape == (5, 31, 17, 3) and e32 < 1e-6, e32
    x = C.encode_inputs(5, 9, 17, 3, seed=4)
    zref, ez = C.encode_reference(m, None, x)
    assert zref.shape == (5, 17, 96) and ez < 1e-6, ez
    with pytest.raises(AssertionError):  # typed weights need their node types
        O.gru_decode(C.state(C.build("freeman17", 96, 96)[0]), None, x2, h, 2)


# ---- the inputs can tell a wrong kernel from a right one ----------------------------------------

def _swap_types(types):
    t = np.array(types).copy()
    i = 0
    j = next(k for k in range(1, len(t)) if t[k] != t[i])
    t[i], t[j] = t[j], t[i]
    return t


def _zeroed(sd, key, index):
    sd = dict(sd)
    w = sd[key].clone()
    w[index] = 0.0
    sd[key] = w
    return sd


CELL = "decoder.rnn.layers.0."


def _decoder_errors(sd, types, x2, h, ph, H):
    """name -> the oracle's output with one deliberate error."""
    dec = lambda s=sd, t=types, x=x2: O.gru_decode(s, t, x, h, ph)  # noqa: E731
    no_add = dict(sd)
    no_add[CELL + "G_add"] = torch.zeros_like(sd[CELL + "G_add"])
    return {
        "G_add dropped": dec(no_add),
        "two node types swapped": dec(t=_swap_types(types)),
        "n-gate third of bias_hh zeroed": dec(_zeroed(sd, CELL + "bias_hh", (Ellipsis, slice(2 * H, None)))),
        "fc.bias zeroed": dec(_zeroed(sd, "decoder.fc.bias", Ellipsis)),
        "x_prev and x_last swapped": dec(x=x2.flip(1)),
        "third frame column of weight_ih zeroed": dec(_zeroed(sd, CELL + "weight_ih", (Ellipsis, 2))),
        "last k-column of weight_hh zeroed": dec(_zeroed(sd, CELL + "weight_hh", (Ellipsis, -1))),
        "last column of the cell's G zeroed": dec(_zeroed(sd, CELL + "G", (slice(None), -1))),
        "last column of fc.G zeroed": dec(_zeroed(sd, "decoder.fc.G", (slice(None), -1))),
    }


@pytest.mark.parametrize("skel", ["h36m16", "amass21", "mano51"])
def test_fixture_detects_deliberate_errors(skel):
    """H = L = 96, B = 5, ph = 7 (decode) / T = 9 (encode): each error shifts the float64 oracle by
    at least 10 times the tolerance the device result of that case is held to."""
    m, types, x2, h, ref, e32 = C.decode_case(skel, 96, 96, 3, 5, 7)
    sd = C.state(m)
    tol = C.tolerance(e32)
    print(f"\n[fixture-guard] {skel} decode: e32 = {e32:.3e}, tolerance = {tol:.3e}")
    for name, out in _decoder_errors(sd, types, x2, h, 7, 96).items():
        shift = C.maxdiff(out, ref)
        print(f"[fixture-guard]   {name}: shift = {shift:.3e} = {shift / tol:.0f} x tolerance")
        assert shift >= 10 * tol, (name, shift, tol)
    m, types, x, zref, ez = C.encode_case(skel, 96, 96, 3, 5, 9)
    sd = C.state(m)
    tol = C.tolerance(ez)
    print(f"[fixture-guard] {skel} encode: e32 = {ez:.3e}, tolerance = {tol:.3e}")
    x_rep = x.clone()
    x_rep[:, 3] = x[:, 4]
    errors = {
        "frame 3 replaced by frame 4": O.gru_encode(sd, types, x_rep),
        "last column of the cell's G zeroed": O.gru_encode(_zeroed(sd, "encoder.rnn.layers.0.G", (slice(None), -1)), types, x),
    }
    for name, out in errors.items():
        shift = C.maxdiff(out, zref)
        print(f"[fixture-guard]   {name}: shift = {shift:.3e} = {shift / tol:.0f} x tolerance")
        assert shift >= 10 * tol, (name, shift, tol)


# ---- ABI validation before any device work -------------------------------------------------------

class _Fn:
    """sd_gru_decode or sd_gru_encode with dummy (never dereferenced) buffers."""

    def __init__(self, which):
        self.L = _lib.lib()
        self.which = which
        self.ws_bytes = getattr(self.L, f"sd_gru_{which}_workspace_bytes")

    def bytes(self, d, rows=4, n=3):
        return int(self.ws_bytes(None if d is None else ctypes.byref(d), rows, n))

    def run(self, d, rows=4, n=3, ws=C.DUMMY, ws_bytes=1 << 40, buf=C.DUMMY):
        dp = None if d is None else ctypes.byref(d)
        if self.which == "decode":
            return self.L.sd_gru_decode(dp, buf, buf, rows, n, buf, ws, ws_bytes, None)
        return self.L.sd_gru_encode(dp, buf, rows, n, buf, ws, ws_bytes, None)

    def err(self):
        return self.L.sd_last_error().decode()

    def desc(self, **kw):
        d, keep = C.desc(**kw)
        if self.which == "encode" and "G_add" not in kw:
            d.G_add = None
        return d, keep


TENSORS = ("init_G", "init_weight", "G", "weight_ih", "weight_hh", "fc_G", "fc_weight")


@pytest.mark.parametrize("which", ["decode", "encode"])
def test_descriptor_validation_on_host(which):
    """A bad descriptor: workspace_bytes returns 0, the call returns SD_E_INVALID and sd_last_error()
    names the field; nothing is dereferenced (every pointer is a dummy)."""
    f = _Fn(which)
    bad = [(None, "descriptor")]
    bad += [(f.desc(J=J)[0], "num_nodes") for J in (0, 65)]
    bad += [(f.desc(F=F)[0], "feature_size") for F in (0, 17)]
    bad += [(f.desc(L=v)[0], "latent_size") for v in (0, 8, 24)]
    bad += [(f.desc(H=v)[0], "hidden_size") for v in (0, 8, 24)]
    bad += [(f.desc(num_node_types=3)[0], "node_types")]
    typed_bad, keep = f.desc(J=16, num_node_types=3, types=[0, 1, 2] * 5 + [3])
    bad += [(typed_bad, "node_types")]
    typed_neg, keep2 = f.desc(J=16, num_node_types=3, types=[0, 1, 2] * 5 + [-1])
    bad += [(typed_neg, "node_types")]
    bad += [(f.desc(**{t: None})[0], t) for t in TENSORS]
    # the gate kernel's LDS: J = 64 with H = 256 needs (3 * 64 * 256 + 64 * 64) * 4 = 208 KB
    bad += [(f.desc(J=64, H=256)[0], "num_nodes"), (f.desc(J=64, H=256)[0], "hidden_size")]
    for d, field in bad:
        assert f.bytes(d) == 0, field
        assert field in f.err(), (field, f.err())
        assert f.run(d) == SD_E_INVALID, field
        assert field in f.err(), (field, f.err())
    # accepted: the largest skeleton at the release width, typed weights with valid types
    assert f.bytes(f.desc(J=64, H=96)[0]) > 0
    assert f.bytes(f.desc(J=64, H=192)[0]) > 0      # (3 * 64 * 192 + 64 * 64) * 4 = 160 KB exactly
    assert f.bytes(f.desc(J=64, H=208)[0]) == 0
    ok_typed, keep3 = f.desc(J=16, num_node_types=3, types=[0, 1, 2] * 5 + [2])
    assert f.bytes(ok_typed) > 0
    # the optional tensors may be NULL
    assert f.bytes(f.desc(init_bias=None, bias_ih=None, bias_hh=None, fc_bias=None, G_add=None)[0]) > 0


@pytest.mark.parametrize("which", ["decode", "encode"])
def test_shape_and_workspace_validation_on_host(which):
    f = _Fn(which)
    d, _ = f.desc(J=21)
    n_name = "ph" if which == "decode" else "frames"
    assert f.bytes(d, rows=-1) == 0 and "rows" in f.err()
    assert f.run(d, rows=-1) == SD_E_INVALID and "rows" in f.err()
    for n in (0, -2):
        assert f.bytes(d, n=n) == 0 and n_name in f.err()
        assert f.run(d, n=n) == SD_E_INVALID and n_name in f.err()
    # an empty batch is a no-op: no buffer is looked at
    assert f.run(d, rows=0, ws=None, ws_bytes=0, buf=None) == SD_OK
    assert f.bytes(d, rows=0) > 0
    # null buffers, a missing workspace, and one byte short of the size workspace_bytes reports
    need = f.bytes(d, rows=5, n=7)
    assert need > 0
    assert f.run(d, rows=5, n=7, buf=None) == SD_E_INVALID and "null" in f.err()
    assert f.run(d, rows=5, n=7, ws=None, ws_bytes=need) == SD_E_INVALID and "workspace" in f.err()
    assert f.run(d, rows=5, n=7, ws=C.DUMMY, ws_bytes=need - 1) == SD_E_INVALID
    assert "workspace" in f.err() and str(need) in f.err(), f.err()
    # monotone in rows and in the number of frames
    assert f.bytes(d, rows=6, n=7) > need
    assert f.bytes(d, rows=5, n=8) > need
    assert f.bytes(d, rows=500, n=7) > f.bytes(d, rows=6, n=7)


def test_encoder_refuses_additive_influence_on_host():
    f = _Fn("encode")
    d, _ = f.desc(J=21, G_add=C.DUMMY)
    assert f.bytes(d, rows=5, n=7) > 0  # the descriptor itself is well-formed (the decoder's)
    assert f.run(d, rows=5, n=7) == SD_E_INVALID and "G_add" in f.err()
