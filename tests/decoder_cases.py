"""Shared fixtures of tests/test_gpu_decoder_shapes.py and tests/test_decoder_host.py: AutoEncoder
modules at other shapes than the H36M one of tests/test_autoencoder.py, their inputs, the float64
oracle and the fp32 CPU module path it is measured against, and the `sd_gru_decoder_desc` built
by hand for calls through the C ABI.

Tolerance of a device result (see tolerance()): e32 is the deviation of the CPU fp32 torch module
path from the float64 oracle on the same inputs, i.e. what fp32 rounding alone does to this
computation with torch's blocked dot products.  The MFMA kernels accumulate K <= 208 terms in
sequence (about sqrt(K) ~ 14 times the rounding of a blocked sum), times roughly 10 for the
device's expf / tanhf and up to 120 recurrent steps of a contracting map: 200 e32.  The floor 2e-6
is 16 fp32 ulps at 1.0, for cases whose e32 happens to be near zero; the project's 1e-4 caps it."""
import ctypes
import functools

import numpy as np
import torch

import oracle as O
from skeletondiffusion_amd import _lib, synthetic
from skeletondiffusion_amd.skeletons import skeleton

SEED = 4321
E32_FACTOR, TOL_FLOOR, TOL_CAP = 200.0, 2e-6, 1e-4


def node_types(skel):
    """A skeleton key, ("mod", J, k) for the types arange(J) % k, or ("none", J) for shared weights
    -> (J, int64 types or None)."""
    if isinstance(skel, str):
        types = skeleton(skel)[3]
        return len(types), types
    if skel[0] == "none":
        return skel[1], None
    _, J, k = skel
    return J, (np.arange(J) % k).astype(np.int64)


def untyped(skel):
    return ("none", node_types(skel)[0])


def build(skel, H, L, F=3, seed=SEED):
    """(AutoEncoder on the CPU in eval mode with the synthetic filler's weights, node types)."""
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    J, types = node_types(skel)
    m = AutoEncoder(num_nodes=J, encoder_hidden_size=H, decoder_hidden_size=H, latent_size=L, input_size=F,
                    node_types=None if types is None else torch.from_numpy(types), z_activation="tanh",
                    enc_num_layers=1, output_size=F, recurrent_arch_enc="StaticGraphGRU",
                    recurrent_arch_decoder="StaticGraphGRU", if_consider_hip=False).eval()
    synthetic.fill_module_(m, seed)
    return m, types


def state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def decode_inputs(B, J, F, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, 2, J, F), generator=g) * 0.3, torch.rand((B, J, L), generator=g) * 2 - 1


def encode_inputs(B, T, J, F, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, T, J, F), generator=g) * 0.3


def tolerance(e32):
    return min(max(E32_FACTOR * e32, TOL_FLOOR), TOL_CAP)


def maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


def decode_reference(m, types, x2, h, ph):
    """(float64 oracle result, e32) of a CPU module."""
    ref = O.gru_decode(state(m), types, x2, h, ph)
    with torch.no_grad():
        cpu, _ = m.decoder(x=x2, h=h, z=None, ph=ph)
    return ref, maxdiff(cpu, ref)


def encode_reference(m, types, x):
    ref = O.gru_encode(state(m), types, x)
    with torch.no_grad():
        cpu = m.z_activation(m(x))
    return ref, maxdiff(cpu, ref)


@functools.lru_cache(maxsize=None)
def decode_case(skel, H, L, F, B, ph):
    """One decode case, computed once per session and never modified: (module on the CPU, types,
    x2, h, oracle result, e32)."""
    m, types = build(skel, H, L, F)
    x2, h = decode_inputs(B, m.decoder.rnn.layers[0].num_nodes, F, L, seed=1000 + 7 * B + ph)
    ref, e32 = decode_reference(m, types, x2, h, ph)
    return m, types, x2, h, ref, e32


@functools.lru_cache(maxsize=None)
def encode_case(skel, H, L, F, B, T):
    m, types = build(skel, H, L, F)
    x = encode_inputs(B, T, m.encoder.rnn.layers[0].num_nodes, F, seed=2000 + 7 * B + T)
    ref, e32 = encode_reference(m, types, x)
    return m, types, x, ref, e32


def report(what, e32, err, tol):
    """The figures of one case, printed before the assertion (profiles/decoder_parity/pytest_gpu.txt)."""
    ratio = err / e32 if e32 > 0 else float("inf")
    print(f"\n[decoder-parity] {what}: e32 = {e32:.3e}  device error = {err:.3e}  ratio = {ratio:.1f}  "
          f"tolerance = {tol:.3e}")


# ---- the C ABI by hand ---------------------------------------------------------------------------

DUMMY = 0x1000  # a non-null pointer for arguments the validation never dereferences


def desc(J=16, F=3, L=96, H=96, num_node_types=0, types=None, ptr=DUMMY, **over):
    """An sd_gru_decoder_desc with every tensor pointer `ptr`, then the overrides; returns (desc,
    objects to keep alive)."""
    d = _lib.SDGruDecoderDesc()
    d.num_nodes, d.feature_size, d.latent_size, d.hidden_size, d.num_node_types = J, F, L, H, num_node_types
    keep = []
    if types is not None:
        arr = (ctypes.c_int64 * len(types))(*[int(t) for t in types])
        keep.append(arr)
        d.node_types = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64))
    for name in ("init_G", "init_weight", "init_bias", "G", "G_add", "weight_ih", "weight_hh", "bias_ih", "bias_hh",
                 "fc_G", "fc_weight", "fc_bias"):
        setattr(d, name, ptr)
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


def module_desc(m, which, dev):
    """The descriptor of a module's decoder ("dec") or encoder ("enc") as DecoderEngine builds it,
    with the tensors on `dev`; returns (desc, keep)."""
    keep = []

    def p(t):
        if t is None or not torch.is_tensor(t):
            return None
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        keep.append(t)
        return t.data_ptr()

    d = _lib.SDGruDecoderDesc()
    if which == "dec":
        net, ih = m.decoder, m.decoder.initial_hidden_h
        cell = net.rnn.layers[0]
        d.feature_size = net.fc.out_features
        d.latent_size = cell.input_size - d.feature_size
        d.G_add = p(cell.G_add)
    else:
        net, ih = m.encoder, m.encoder.initial_hidden1
        cell = net.rnn.layers[0]
        d.feature_size, d.latent_size = cell.input_size, net.fc.out_features
        d.G_add = None
    J = cell.num_nodes
    d.num_nodes, d.hidden_size = J, cell.hidden_size
    nt = cell.node_type_index
    if nt is not None:
        arr = (ctypes.c_int64 * J)(*[int(v) for v in nt.tolist()])
        keep.append(arr)
        d.num_node_types = int(cell.weight_hh.shape[0])
        d.node_types = ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64))
    d.init_G, d.init_weight, d.init_bias = p(ih.G), p(ih.weight), p(ih.bias)
    d.G = p(cell.G)
    d.weight_ih, d.weight_hh, d.bias_ih, d.bias_hh = p(cell.weight_ih), p(cell.weight_hh), p(cell.bias_ih), p(cell.bias_hh)
    d.fc_G, d.fc_weight, d.fc_bias = p(net.fc.G), p(net.fc.weight), p(net.fc.bias)
    return d, keep
