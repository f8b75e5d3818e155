"""Training-side StaticGraphLinear on HIP (SURVEY.md §8f "next" #4).

`GraphLinearFunction` is a torch.autograd.Function whose forward and backward are the
`sd_gl_train_forward` / `sd_gl_train_backward` kernels (include/skeldiff.h,
csrc/sd_train.hip).  It replaces, for fp32 device tensors under autograd, the einsum/matmul
forward of the reference's GraphLinear (src/core/network/layers/graph_structural.py:30-43,
StaticGraphLinear :105-114) and the backward torch derives for it when
`NonisotropicGaussianDiffusion.forward` trains the Denoiser (src/core/diffusion/base.py:262-307,
src/core/trainer.py:224-276).  The mixing matrix's own gradient flows on through torch into G
(Ghat = G / rowsum|G| is a J x J torch op).

`StaticGraphLinear.forward` (core/network/layers.py) routes here when the input is an fp32 device
tensor, grad is enabled and `hip_training_enabled()`; there is no silent CPU fallback on a GPU
(the library must load or the call raises).

`graph_gru` / `gx_table` are the graph-GRU sequence core and its per-step mixing matrices for
stage-1 training of the motion autoencoder (`sd_gru_train_*`, `sd_gx_table_*`,
csrc/sd_gru_train.hip), under the same switch.
`graph_lstm` is the same for StaticGraphLSTM encoders / decoders (`sd_lstm_train_*`,
csrc/sd_lstm_train.hip).

`hip_forward_only()` lets the same forward kernels serve a forward under `no_grad`, and
`q_sample_groups` is the forward process for k noisy copies per sequence (`sd_q_sample_groups`,
csrc/sd_q_sample.hip): the two pieces of the selected-row best-of-k step (core/best_of_k.py,
DESIGN.md §4w).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import threading
from typing import Optional

import torch

from . import _lib

_ENABLED = True


def set_hip_training(enabled: bool) -> bool:
    """Switch the HIP training graph-linear on/off (process-wide).  Returns the previous value."""
    global _ENABLED
    prev, _ENABLED = _ENABLED, bool(enabled)
    return prev


def hip_training_enabled() -> bool:
    return _ENABLED


_FORWARD_ONLY = threading.local()


@contextlib.contextmanager
def hip_forward_only():
    """While active (this thread only), the HIP training kernels also serve forwards that run with
    grad disabled: every gate that reads `hip_gate()` passes under `torch.no_grad()`, the same
    forward kernels run and autograd keeps nothing for a backward.  Off by default; with it off
    every gate evaluates exactly as `torch.is_grad_enabled()`."""
    prev = getattr(_FORWARD_ONLY, "on", False)
    _FORWARD_ONLY.on = True
    try:
        yield
    finally:
        _FORWARD_ONLY.on = prev


def hip_forward_only_active() -> bool:
    return getattr(_FORWARD_ONLY, "on", False)


def hip_gate() -> bool:
    """The autograd condition of every HIP training gate: grad enabled, or `hip_forward_only()`."""
    return torch.is_grad_enabled() or getattr(_FORWARD_ONLY, "on", False)


MAX_NODES = 64  # sd_gl_train_forward / _backward: 1 <= J <= 64


def hip_shapes_ok(x, weight, ghat, node_types) -> bool:
    """Whether a StaticGraphLinear call fits the HIP training kernels (else the torch path
    runs): J <= 64, a (J, J) mixing matrix, and a node_types vector of length J whose values
    index the weight's type axis.  Mismatches raise the torch path's own shape errors instead of
    becoming out-of-bounds device reads."""
    if x.dim() < 2:
        return False
    J = x.shape[-2]
    if not (1 <= J <= MAX_NODES) or tuple(ghat.shape) != (J, J) or weight.dim() not in (2, 3):
        return False
    if node_types is None:
        return weight.dim() == 2
    if weight.dim() != 3 or node_types.numel() != J:
        return False
    nt = node_types.detach()
    return bool((nt >= 0).all()) and int(nt.max()) < weight.shape[0]


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


class GraphLinearFunction(torch.autograd.Function):
    """y = ghat @ (W[type j] x_j + bias[type j]) with the backward on HIP.

    x (..., J, K); weight (types, N, K) or (N, K) (shared); bias (types, N), (N,) or None;
    ghat (J, J); node_types (J,) int64 on the device or None (shared weights)."""

    @staticmethod
    def forward(ctx, x, weight, bias, ghat, node_types):
        J, K = x.shape[-2], x.shape[-1]
        lead = x.shape[:-2]
        xc = x.reshape(-1, J, K).contiguous()
        w3 = weight if weight.dim() == 3 else weight.unsqueeze(0)
        w3 = w3.contiguous()
        n_types = int(w3.shape[0]) if node_types is not None else 0
        N = int(w3.shape[1])
        if w3.shape[2] != K:
            raise ValueError(f"weight in_features {w3.shape[2]} != input features {K}")
        b2 = None if bias is None else bias.reshape(w3.shape[0], N).contiguous()
        gh = ghat.contiguous()
        nt = None if node_types is None else node_types.to(device=x.device, dtype=torch.int64).contiguous()
        rows = xc.shape[0]
        z = torch.empty(rows, J, N, device=x.device, dtype=torch.float32)
        y = torch.empty_like(z)
        _lib.check(_lib.lib().sd_gl_train_forward(
            xc.data_ptr(), w3.data_ptr(), _lib.ptr(b2), _lib.ptr(nt), n_types, gh.data_ptr(), rows, J, K, N,
            z.data_ptr(), y.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(xc, z, w3, gh, nt)
        ctx.meta = (lead, J, K, N, n_types, weight.shape, None if bias is None else bias.shape)
        return y.reshape(*lead, J, N)

    @staticmethod
    def backward(ctx, dy):
        xc, z, w3, gh, nt = ctx.saved_tensors
        lead, J, K, N, n_types, wshape, bshape = ctx.meta
        need_x, need_w, need_b, need_g, _ = ctx.needs_input_grad
        dyc = dy.reshape(-1, J, N).contiguous().float()
        rows = dyc.shape[0]
        dev = dyc.device
        dx = torch.empty(rows, J, K, device=dev) if need_x else None
        dW = torch.empty(w3.shape, device=dev) if need_w else None
        db = torch.empty(w3.shape[0], N, device=dev) if (need_b and bshape is not None) else None
        dg = torch.empty(J, J, device=dev) if need_g else None
        L = _lib.lib()
        ws_bytes = L.sd_gl_train_workspace_bytes(rows, J, K, N, n_types)
        ws = torch.empty((ws_bytes + 3) // 4, device=dev, dtype=torch.float32)
        _lib.check(L.sd_gl_train_backward(
            xc.data_ptr(), z.data_ptr(), dyc.data_ptr(), w3.data_ptr(), _lib.ptr(nt), n_types, gh.data_ptr(), rows,
            J, K, N, _lib.ptr(dx), _lib.ptr(dW), _lib.ptr(db), _lib.ptr(dg), ws.data_ptr(), ws_bytes, _stream(dev)))
        return (None if dx is None else dx.reshape(*lead, J, K),
                None if dW is None else dW.reshape(wshape),
                None if db is None else db.reshape(bshape),
                dg, None)


class AttentionCoreFunction(torch.autograd.Function):
    """out = softmax((q scale) k^T) v per head over the joint axis, from to_qkv's output
    (reference attention.py:122-136, without dropout / q-k norms), forward and backward on HIP
    (`sd_attn_train_forward` / `_backward`, csrc/sd_train.hip).  qkv (..., J, 3 * heads * dim_head)
    -> (..., J, heads * dim_head)."""

    @staticmethod
    def forward(ctx, qkv, heads: int, dim_head: int, scale: float):
        J, W = qkv.shape[-2], qkv.shape[-1]
        if W != 3 * heads * dim_head:
            raise ValueError(f"qkv width {W} != 3 * {heads} * {dim_head}")
        lead = qkv.shape[:-2]
        qc = qkv.reshape(-1, J, W).contiguous()
        rows = qc.shape[0]
        out = torch.empty(rows, J, heads * dim_head, device=qkv.device, dtype=torch.float32)
        _lib.check(_lib.lib().sd_attn_train_forward(qc.data_ptr(), out.data_ptr(), rows, J, heads, dim_head,
                                                     float(scale), _stream(qkv.device)))
        ctx.save_for_backward(qc)
        ctx.meta = (lead, J, heads, dim_head, float(scale))
        return out.reshape(*lead, J, heads * dim_head)

    @staticmethod
    def backward(ctx, dout):
        (qc,) = ctx.saved_tensors
        lead, J, heads, dim_head, scale = ctx.meta
        dc = dout.reshape(-1, J, heads * dim_head).contiguous().float()
        dqkv = torch.empty_like(qc)
        _lib.check(_lib.lib().sd_attn_train_backward(qc.data_ptr(), dc.data_ptr(), dqkv.data_ptr(), qc.shape[0], J,
                                                      heads, dim_head, scale, _stream(qc.device)))
        return dqkv.reshape(*lead, J, 3 * heads * dim_head), None, None, None


def attention_core(qkv: torch.Tensor, heads: int, dim_head: int, scale: float) -> torch.Tensor:
    """HIP attention core under autograd (fp32 device tensors, J <= 64, dim_head <= 64)."""
    if not qkv.is_cuda or qkv.dtype != torch.float32:
        raise ValueError("attention_core: the HIP training path needs fp32 device tensors")
    return AttentionCoreFunction.apply(qkv, heads, dim_head, scale)


class FilmTanhFunction(torch.autograd.Function):
    """tanh(y (scale + 1) + shift) with (scale | shift) = ss (rows, 1, 2C) broadcast over the J
    nodes -- a ResnetBlock's first Block after its graph-linear (reference attention.py:67-75) --
    forward and backward on HIP (`sd_film_tanh_forward` / `_backward`)."""

    @staticmethod
    def forward(ctx, y, ss):
        rows, J, C = y.shape
        yc = y.contiguous()
        sc = ss.reshape(rows, 2 * C).contiguous()
        out = torch.empty_like(yc)
        _lib.check(_lib.lib().sd_film_tanh_forward(yc.data_ptr(), sc.data_ptr(), out.data_ptr(), rows, J, C,
                                                    _stream(y.device)))
        ctx.save_for_backward(yc, sc, out)
        ctx.ss_shape = ss.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        yc, sc, out = ctx.saved_tensors
        rows, J, C = yc.shape
        dc = dout.contiguous().float()
        dy = torch.empty_like(yc)
        dss = torch.empty_like(sc)
        _lib.check(_lib.lib().sd_film_tanh_backward(yc.data_ptr(), sc.data_ptr(), out.data_ptr(), dc.data_ptr(),
                                                     dy.data_ptr(), dss.data_ptr(), rows, J, C, _stream(yc.device)))
        return dy, dss.reshape(ctx.ss_shape)


def film_tanh(y: torch.Tensor, ss: torch.Tensor) -> torch.Tensor:
    """HIP FiLM + tanh under autograd: y (rows, J, C) fp32 on the device, ss (rows, 1, 2C)."""
    if not y.is_cuda or y.dtype != torch.float32 or ss.dtype != torch.float32:
        raise ValueError("film_tanh: the HIP training path needs fp32 device tensors")
    return FilmTanhFunction.apply(y, ss)


def graph_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], ghat: torch.Tensor,
                 node_types: Optional[torch.Tensor]) -> torch.Tensor:
    """HIP StaticGraphLinear under autograd (fp32 device tensors)."""
    if not x.is_cuda:
        raise ValueError("graph_linear: the HIP training path needs device tensors")
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise ValueError("graph_linear: the HIP training path is fp32")
    return GraphLinearFunction.apply(x, weight, bias, ghat, node_types)


# ---- graph-GRU sequence core and gx table (reference recurrent.py:321-391) -------

# launches of the sequence entries since import, by name (tests and tools read it as a spy)
CALLS = collections.Counter()

# forwards of the sequence cores that kept their backward's state, by cell ("gru", "lstm")
STATE_KEPT = collections.Counter()

GRU_MAX_HIDDEN = 256  # sd_gru_train_*: H a positive multiple of 16, at most 256


def _host_types(node_types, J: int):
    """ctypes int64 array (or None) of a node-type vector for the entries that take it on the
    host; one device-to-host copy per (tensor, version), not one per call."""
    if node_types is None:
        return None
    key = (id(node_types), node_types._version)
    hit = _HOST_TYPES.get(key)
    if hit is None or hit[0] is not node_types:
        vals = [int(v) for v in node_types.detach().cpu().reshape(-1).tolist()]
        if len(vals) != J:
            raise ValueError(f"node_types has {len(vals)} entries, the input {J} nodes")
        if len(_HOST_TYPES) > 64:
            _HOST_TYPES.clear()
        hit = (node_types, (ctypes.c_int64 * J)(*vals))
        _HOST_TYPES[key] = hit
    return hit[1]


_HOST_TYPES: dict = {}


def _keeps_state(*tensors) -> bool:
    """Whether a sequence forward keeps the state its backward reads: grad mode is on and an input
    asks for a gradient.  Decided outside the Function: inside its forward, `ctx.needs_input_grad`
    is True for every `requires_grad` input (the Parameters) under `no_grad` too."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class GraphGRUFunction(torch.autograd.Function):
    """hs = the StaticGraphGRU cell unrolled over T steps from the unmixed input projections
    (`sd_gru_train_forward` / `_backward`, csrc/sd_gru_train.hip).  The state backward reads is
    kept only when `keep` (`_keeps_state`: under no_grad the same forward runs without it)."""

    @staticmethod
    def forward(ctx, a, h0, gx, weight_hh, bias_hh, node_types, T: int, keep: bool):
        B, Ta, J, H3 = a.shape
        H = H3 // 3
        Tg = gx.shape[0]
        ac, hc, gc = a.contiguous(), h0.contiguous(), gx.contiguous()
        w3 = (weight_hh if weight_hh.dim() == 3 else weight_hh.unsqueeze(0)).contiguous()
        n_types = int(w3.shape[0]) if node_types is not None else 0
        b2 = None if bias_hh is None else bias_hh.reshape(w3.shape[0], H3).contiguous()
        nt = _host_types(node_types, J)
        dev = a.device
        hs = torch.empty(B, T, J, H, device=dev, dtype=torch.float32)
        hprev = torch.empty_like(hs) if keep else None
        c = torch.empty(B, T, J, H3, device=dev, dtype=torch.float32) if keep else None
        gates = torch.empty(B, T, J, 4 * H, device=dev, dtype=torch.float32) if keep else None
        L = _lib.lib()
        ws_bytes = L.sd_gru_train_workspace_bytes(B, T, J, H, n_types)
        ws = torch.empty(max(1, (ws_bytes + 3) // 4), device=dev, dtype=torch.float32)
        CALLS["gru_forward"] += 1
        STATE_KEPT["gru"] += int(keep)
        _lib.check(L.sd_gru_train_forward(
            ac.data_ptr(), Ta, hc.data_ptr(), gc.data_ptr(), Tg, w3.data_ptr(), _lib.ptr(b2), nt, n_types, B, T, J, H,
            hs.data_ptr(), _lib.ptr(hprev), _lib.ptr(c), _lib.ptr(gates), ws.data_ptr(), ws_bytes, _stream(dev)))
        if keep:
            ctx.save_for_backward(ac, gc, w3, hprev, c, gates)
            ctx.meta = (B, T, Ta, Tg, J, H, n_types, nt, weight_hh.shape, None if bias_hh is None else bias_hh.shape,
                        a.shape, h0.shape, gx.shape)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        ac, gc, w3, hprev, c, gates = ctx.saved_tensors
        B, T, Ta, Tg, J, H, n_types, nt, wshape, bshape, ashape, hshape, gshape = ctx.meta
        need_a, need_h, need_g, need_w, need_b = ctx.needs_input_grad[:5]
        dev = ac.device
        dc = dhs.contiguous().float()
        da = torch.empty(B, Ta, J, 3 * H, device=dev) if need_a else None
        dh0 = torch.empty(B, J, H, device=dev) if need_h else None
        dgx = torch.empty(Tg, J, J, device=dev) if need_g else None
        dW = torch.empty(w3.shape, device=dev) if need_w else None
        db = torch.empty(w3.shape[0], 3 * H, device=dev) if (need_b and bshape is not None) else None
        L = _lib.lib()
        ws_bytes = L.sd_gru_train_workspace_bytes(B, T, J, H, n_types)
        ws = torch.empty(max(1, (ws_bytes + 3) // 4), device=dev, dtype=torch.float32)
        CALLS["gru_backward"] += 1
        _lib.check(L.sd_gru_train_backward(
            dc.data_ptr(), ac.data_ptr(), Ta, gc.data_ptr(), Tg, w3.data_ptr(), nt, n_types, hprev.data_ptr(),
            c.data_ptr(), gates.data_ptr(), B, T, J, H, _lib.ptr(da), _lib.ptr(dh0), _lib.ptr(dgx), _lib.ptr(dW),
            _lib.ptr(db), ws.data_ptr(), ws_bytes, _stream(dev)))
        return (None if da is None else da.reshape(ashape), None if dh0 is None else dh0.reshape(hshape),
                None if dgx is None else dgx.reshape(gshape), None if dW is None else dW.reshape(wshape),
                None if db is None else db.reshape(bshape), None, None, None)


def graph_gru(a: torch.Tensor, h0: torch.Tensor, gx: torch.Tensor, weight_hh: torch.Tensor,
              bias_hh: Optional[torch.Tensor], node_types: Optional[torch.Tensor],
              steps: Optional[int] = None) -> torch.Tensor:
    """HIP graph-GRU core under autograd (fp32 device tensors; recurrent.py:321-366 unrolled,
    clockwork off).  a (B, Ta, J, 3H) = the unmixed input projections W_ih x + b_ih, Ta = T or 1
    (one projection reused at every step); h0 (B, J, H); gx (Tg, J, J) or (J, J), Tg = T or 1;
    weight_hh (types, 3H, H) with node_types (J,), or (3H, H) shared with node_types None; bias_hh
    or None.  `steps` = T (default: the larger of Ta and Tg).  Returns hs (B, T, J, H)."""
    if not a.is_cuda or a.dtype != torch.float32 or weight_hh.dtype != torch.float32 or h0.dtype != torch.float32 \
            or gx.dtype != torch.float32:
        raise ValueError("graph_gru: the HIP training path needs fp32 device tensors")
    if a.dim() != 4 or a.shape[-1] % 3 or h0.dim() != 3:
        raise ValueError("graph_gru: a (B, Ta, J, 3H) and h0 (B, J, H)")
    if gx.dim() == 2:
        gx = gx.unsqueeze(0)
    B, Ta, J, H3 = a.shape
    H = H3 // 3
    T = int(steps) if steps is not None else max(Ta, gx.shape[0])
    if tuple(h0.shape) != (B, J, H) or gx.dim() != 3 or tuple(gx.shape[1:]) != (J, J):
        raise ValueError("graph_gru: h0 must be (B, J, H) and gx (Tg, J, J)")
    if (node_types is None) != (weight_hh.dim() == 2) or tuple(weight_hh.shape[-2:]) != (H3, H):
        raise ValueError("graph_gru: weight_hh (types, 3H, H) with node_types, or (3H, H) without")
    if bias_hh is not None and bias_hh.numel() != weight_hh.numel() // H:
        raise ValueError("graph_gru: bias_hh must hold 3H values per weight type")
    return GraphGRUFunction.apply(a, h0, gx, weight_hh, bias_hh, node_types, T,
                                  _keeps_state(a, h0, gx, weight_hh, bias_hh))


# ---- graph-LSTM sequence core (reference recurrent.py:126-196) --------------------

# launches of the LSTM sequence entries since import, by name (a counter of its own: CALLS holds
# the GRU path's names only)
LSTM_CALLS = collections.Counter()

LSTM_MAX_HIDDEN = 256  # sd_lstm_train_*: H a positive multiple of 16, at most 256


class GraphLSTMFunction(torch.autograd.Function):
    """(hs, s_last) = the StaticGraphLSTM cell unrolled over T steps from the unmixed input
    projections (`sd_lstm_train_forward` / `_backward`, csrc/sd_lstm_train.hip).  The state backward
    reads is kept only when `keep` (`_keeps_state`); without it the same forward runs, allocates
    neither P, gates nor the cell states, and takes the forward-only workspace.  s_last is not
    differentiable."""

    @staticmethod
    def forward(ctx, a, h0, s0, gx, weight_hh, bias_hh, node_types, T: int, keep: bool):
        B, Ta, J, H4 = a.shape
        H = H4 // 4
        Tg = gx.shape[0]
        ac, hc, sc, gc = a.contiguous(), h0.contiguous(), s0.contiguous(), gx.contiguous()
        w3 = (weight_hh if weight_hh.dim() == 3 else weight_hh.unsqueeze(0)).contiguous()
        n_types = int(w3.shape[0]) if node_types is not None else 0
        b2 = None if bias_hh is None else bias_hh.reshape(w3.shape[0], H4).contiguous()
        nt = _host_types(node_types, J)
        dev = a.device
        hs = torch.empty(B, T, J, H, device=dev, dtype=torch.float32)
        s_last = torch.empty(B, J, H, device=dev, dtype=torch.float32)
        P = torch.empty(B, T, J, H4, device=dev, dtype=torch.float32) if keep else None
        gates = torch.empty(B, T, J, H4, device=dev, dtype=torch.float32) if keep else None
        sseq = torch.empty(B, T, J, H, device=dev, dtype=torch.float32) if keep else None
        L = _lib.lib()
        ws_bytes = L.sd_lstm_train_forward_workspace_bytes(B, J, H, n_types)
        ws = torch.empty(max(1, (ws_bytes + 3) // 4), device=dev, dtype=torch.float32)
        LSTM_CALLS["lstm_forward"] += 1
        STATE_KEPT["lstm"] += int(keep)
        _lib.check(L.sd_lstm_train_forward(
            ac.data_ptr(), Ta, hc.data_ptr(), sc.data_ptr(), gc.data_ptr(), Tg, w3.data_ptr(), _lib.ptr(b2), nt, n_types,
            B, T, J, H, hs.data_ptr(), s_last.data_ptr(), _lib.ptr(P), _lib.ptr(gates), _lib.ptr(sseq), ws.data_ptr(),
            ws_bytes, _stream(dev)))
        if keep:
            ctx.save_for_backward(gc, w3, hc, sc, hs, P, gates, sseq)
            ctx.meta = (B, T, Ta, Tg, J, H, n_types, nt, weight_hh.shape, None if bias_hh is None else bias_hh.shape,
                        a.shape, h0.shape, gx.shape)
        ctx.mark_non_differentiable(s_last)
        return hs, s_last

    @staticmethod
    def backward(ctx, dhs, _ds_last):
        gc, w3, hc, sc, hs, P, gates, sseq = ctx.saved_tensors
        B, T, Ta, Tg, J, H, n_types, nt, wshape, bshape, ashape, hshape, gshape = ctx.meta
        need_a, need_h, need_s, need_g, need_w, need_b = ctx.needs_input_grad[:6]
        dev = gc.device
        dc = dhs.contiguous().float()
        da = torch.empty(B, Ta, J, 4 * H, device=dev) if need_a else None
        dh0 = torch.empty(B, J, H, device=dev) if need_h else None
        ds0 = torch.empty(B, J, H, device=dev) if need_s else None
        dgx = torch.empty(Tg, J, J, device=dev) if need_g else None
        dW = torch.empty(w3.shape, device=dev) if need_w else None
        db = torch.empty(w3.shape[0], 4 * H, device=dev) if (need_b and bshape is not None) else None
        L = _lib.lib()
        ws_bytes = L.sd_lstm_train_workspace_bytes(B, T, J, H, n_types)
        ws = torch.empty(max(1, (ws_bytes + 3) // 4), device=dev, dtype=torch.float32)
        LSTM_CALLS["lstm_backward"] += 1
        _lib.check(L.sd_lstm_train_backward(
            dc.data_ptr(), Ta, gc.data_ptr(), Tg, w3.data_ptr(), nt, n_types, hc.data_ptr(), sc.data_ptr(),
            hs.data_ptr(), P.data_ptr(), gates.data_ptr(), sseq.data_ptr(), B, T, J, H, _lib.ptr(da), _lib.ptr(dh0),
            _lib.ptr(ds0), _lib.ptr(dgx), _lib.ptr(dW), _lib.ptr(db), ws.data_ptr(), ws_bytes, _stream(dev)))
        return (None if da is None else da.reshape(ashape), None if dh0 is None else dh0.reshape(hshape),
                None if ds0 is None else ds0.reshape(hshape), None if dgx is None else dgx.reshape(gshape),
                None if dW is None else dW.reshape(wshape), None if db is None else db.reshape(bshape), None, None, None)


def graph_lstm(a: torch.Tensor, h0: torch.Tensor, s0: torch.Tensor, gx: torch.Tensor, weight_hh: torch.Tensor,
               bias_hh: Optional[torch.Tensor], node_types: Optional[torch.Tensor], steps: Optional[int] = None):
    """HIP graph-LSTM core under autograd (fp32 device tensors; recurrent.py:126-167 unrolled,
    clockwork off).  a (B, Ta, J, 4H) = the unmixed input projections W_ih x (no bias: the cell never
    reads bias_ih), Ta = T or 1 (one projection reused at every step); h0, s0 (B, J, H) the initial
    hidden and cell state; gx (Tg, J, J) or (J, J), Tg = T or 1; weight_hh (types, 4H, H) with
    node_types (J,), or (4H, H) shared with node_types None; bias_hh or None.  `steps` = T (default:
    the larger of Ta and Tg).  Returns (hs (B, T, J, H), s_last (B, J, H)); s_last carries no
    gradient."""
    if not a.is_cuda or any(v.dtype != torch.float32 for v in (a, h0, s0, gx, weight_hh)):
        raise ValueError("graph_lstm: the HIP training path needs fp32 device tensors")
    if a.dim() != 4 or a.shape[-1] % 4 or h0.dim() != 3:
        raise ValueError("graph_lstm: a (B, Ta, J, 4H) and h0 (B, J, H)")
    if gx.dim() == 2:
        gx = gx.unsqueeze(0)
    B, Ta, J, H4 = a.shape
    H = H4 // 4
    T = int(steps) if steps is not None else max(Ta, gx.shape[0])
    if tuple(h0.shape) != (B, J, H) or tuple(s0.shape) != (B, J, H) or gx.dim() != 3 or tuple(gx.shape[1:]) != (J, J):
        raise ValueError("graph_lstm: h0 and s0 must be (B, J, H) and gx (Tg, J, J)")
    if (node_types is None) != (weight_hh.dim() == 2) or tuple(weight_hh.shape[-2:]) != (H4, H):
        raise ValueError("graph_lstm: weight_hh (types, 4H, H) with node_types, or (4H, H) without")
    if bias_hh is not None and bias_hh.numel() != weight_hh.numel() // H:
        raise ValueError("graph_lstm: bias_hh must hold 4H values per weight type")
    return GraphLSTMFunction.apply(a, h0, s0, gx, weight_hh, bias_hh, node_types, T,
                                   _keeps_state(a, h0, s0, gx, weight_hh, bias_hh))


class GxTableFunction(torch.autograd.Function):
    """gxt[0] = normalize_L1(G) or G, gxt[t + 1] = normalize_L1(gxt[t] + G_add), one HIP launch
    each way (`sd_gx_table_forward` / `_backward`)."""

    @staticmethod
    def forward(ctx, G, G_add, steps: int, normalize0: bool, eps: float):
        Gc = G.detach().contiguous()
        Ac = None if G_add is None else G_add.detach().contiguous()
        J = Gc.shape[0]
        out = torch.empty(steps, J, J, device=G.device, dtype=torch.float32)
        CALLS["gx_table_forward"] += 1
        _lib.check(_lib.lib().sd_gx_table_forward(Gc.data_ptr(), _lib.ptr(Ac), J, steps, int(normalize0), float(eps),
                                                  out.data_ptr(), _stream(G.device)))
        ctx.save_for_backward(Gc, Ac, out)
        ctx.meta = (J, steps, int(normalize0), float(eps))
        return out

    @staticmethod
    def backward(ctx, dout):
        Gc, Ac, out = ctx.saved_tensors
        J, steps, normalize0, eps = ctx.meta
        need_add = Ac is not None and ctx.needs_input_grad[1]
        dc = dout.contiguous().float()
        dG = torch.empty_like(Gc)
        dA = torch.empty_like(Gc) if need_add else None
        CALLS["gx_table_backward"] += 1
        _lib.check(_lib.lib().sd_gx_table_backward(Gc.data_ptr(), _lib.ptr(Ac), out.data_ptr(), dc.data_ptr(), J, steps,
                                                   normalize0, eps, dG.data_ptr(), _lib.ptr(dA), _stream(Gc.device)))
        return dG, dA, None, None, None


def gx_table(G: torch.Tensor, G_add: Optional[torch.Tensor], steps: int, normalize0: bool = True,
             eps: float = 1e-12) -> torch.Tensor:
    """HIP table of the GRU cell's mixing matrix over `steps` steps under autograd
    (recurrent.py:333-334, 361-364): (J, J) fp32 device matrices, J <= 64 -> (steps, J, J)."""
    J = G.shape[0]
    if not G.is_cuda or G.dtype != torch.float32 or G.dim() != 2 or tuple(G.shape) != (J, J) or J > MAX_NODES:
        raise ValueError("gx_table: the HIP training path needs a (J, J) fp32 device matrix, J <= 64")
    if G_add is not None and (G_add.dtype != torch.float32 or tuple(G_add.shape) != (J, J) or G_add.device != G.device):
        raise ValueError("gx_table: G_add must match G")
    if steps < 1:
        raise ValueError("gx_table: steps must be >= 1")
    return GxTableFunction.apply(G, G_add, int(steps), bool(normalize0), float(eps))


class L1NormRowsFunction(torch.autograd.Function):
    """Ghat_k = G_k / max(rowsum|G_k|, eps) (F.normalize(G, p=1, dim=1), reference
    graph_structural.py:107) for L matrices G_1 .. G_L of one size, forward and backward on HIP
    (`sd_l1norm_rows_forward` / `_backward`, one launch each way for all L): the Denoiser
    normalises all its learnable G at once per forward instead of torch's norm / clamp / div chain
    and its backward per StaticGraphLinear call.  apply(eps, G_1, ..., G_L) -> (Ghat_1, ..., Ghat_L)."""

    @staticmethod
    def forward(ctx, eps: float, *Gs):
        Gc = torch.stack([g.detach() for g in Gs]).contiguous()
        L, J = Gc.shape[0], Gc.shape[1]
        out = torch.empty_like(Gc)
        _lib.check(_lib.lib().sd_l1norm_rows_forward(Gc.data_ptr(), out.data_ptr(), J, L, float(eps),
                                                      _stream(Gc.device)))
        ctx.save_for_backward(Gc)
        ctx.eps = float(eps)
        return tuple(out.unbind(0))

    @staticmethod
    def backward(ctx, *douts):
        (Gc,) = ctx.saved_tensors
        L, J = Gc.shape[0], Gc.shape[1]
        dc = torch.stack([torch.zeros_like(Gc[0]) if d is None else d.float() for d in douts]).contiguous()
        dG = torch.empty_like(Gc)
        _lib.check(_lib.lib().sd_l1norm_rows_backward(Gc.data_ptr(), dc.data_ptr(), dG.data_ptr(), J, L, ctx.eps,
                                                       _stream(Gc.device)))
        return (None,) + tuple(dG.unbind(0))


def l1norm_rows_many(Gs, eps: float = 1e-12):
    """HIP row-wise L1 normalisation of L (J, J) fp32 device matrices under autograd (J <= 64), one
    launch each way."""
    Gs = list(Gs)
    if not Gs:
        return ()
    J = Gs[0].shape[0]
    for G in Gs:
        if (not G.is_cuda or G.dtype != torch.float32 or G.dim() != 2 or tuple(G.shape) != (J, J)
                or J > MAX_NODES or G.device != Gs[0].device):
            raise ValueError("l1norm_rows: the HIP training path needs (J, J) fp32 device matrices, J <= 64")
    return L1NormRowsFunction.apply(eps, *Gs)


def l1norm_rows(G: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """HIP row-wise L1 normalisation of one (J, J) fp32 device matrix under autograd (J <= 64)."""
    return l1norm_rows_many([G], eps)[0]


class RMSNormFunction(torch.autograd.Function):
    """PreNorm's RMSNorm, x / max(||x||, eps) * g * sqrt(C) over the last axis (reference
    attention.py:30-36), forward and backward on HIP (`sd_rmsnorm_forward` / `_backward`)."""

    @staticmethod
    def forward(ctx, x, g, scale: float, eps: float):
        C = x.shape[-1]
        xc = x.reshape(-1, C).contiguous()
        gc = g.reshape(C).contiguous()
        R = xc.shape[0]
        out = torch.empty_like(xc)
        dnorm = torch.empty(R, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().sd_rmsnorm_forward(xc.data_ptr(), gc.data_ptr(), out.data_ptr(), dnorm.data_ptr(), R, C,
                                                  float(scale), float(eps), _stream(x.device)))
        ctx.save_for_backward(xc, gc, dnorm)
        ctx.meta = (x.shape, g.shape, float(scale), float(eps))
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, dout):
        xc, gc, dnorm = ctx.saved_tensors
        xshape, gshape, scale, eps = ctx.meta
        R, C = xc.shape
        dc = dout.reshape(R, C).contiguous().float()
        dx = torch.empty_like(xc)
        dg = torch.empty(C, device=xc.device, dtype=torch.float32)
        L = _lib.lib()
        ws_bytes = L.sd_rmsnorm_workspace_bytes(R, C)
        ws = torch.empty(max(1, (ws_bytes + 3) // 4), device=xc.device, dtype=torch.float32)
        _lib.check(L.sd_rmsnorm_backward(xc.data_ptr(), gc.data_ptr(), dnorm.data_ptr(), dc.data_ptr(), dx.data_ptr(),
                                         dg.data_ptr(), R, C, scale, eps, ws.data_ptr(), ws_bytes, _stream(xc.device)))
        return dx.reshape(xshape), dg.reshape(gshape), None, None


def rmsnorm(x: torch.Tensor, g: torch.Tensor, scale: float, eps: float = 1e-12) -> torch.Tensor:
    """HIP RMSNorm under autograd: x (..., C) and g (C elements) fp32 on the device, C <= 1024."""
    if not x.is_cuda or x.dtype != torch.float32 or g.dtype != torch.float32 or x.shape[-1] > 1024:
        raise ValueError("rmsnorm: the HIP training path needs fp32 device tensors with C <= 1024")
    return RMSNormFunction.apply(x, g, scale, eps)


class MahalanobisLossFunction(torch.autograd.Function):
    """Per-row Mahalanobis loss of NonisotropicGaussianDiffusion: mean over (J, F) of
    |S[t] D| (l1) or (S[t] D)^2 (mse), D = target - model_out (pred_noise) or model_out - target
    (reference nonisotropic.py:177-190 + the 'b ... -> b' mean of base.py:298), forward and
    backward on HIP (`sd_mahalanobis_loss_forward` / `_backward`).  The target gets the negated
    gradient of model_out."""

    @staticmethod
    def forward(ctx, model_out, target, S, t, pred_noise: bool, mse: bool):
        rows, J, F = model_out.shape
        mo = model_out.contiguous()
        tg = target.contiguous().float()
        Sc = S.contiguous()
        tc = t.to(device=mo.device, dtype=torch.int64).contiguous()
        loss = torch.empty(rows, device=mo.device, dtype=torch.float32)
        _lib.check(_lib.lib().sd_mahalanobis_loss_forward(mo.data_ptr(), tg.data_ptr(), Sc.data_ptr(), tc.data_ptr(),
                                                           Sc.shape[0], rows, J, F, int(pred_noise), int(mse), loss.data_ptr(),
                                                           _stream(mo.device)))
        ctx.save_for_backward(mo, tg, Sc, tc)
        ctx.flags = (int(pred_noise), int(mse))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        mo, tg, Sc, tc = ctx.saved_tensors
        pred_noise, mse = ctx.flags
        rows, J, F = mo.shape
        dl = dloss.contiguous().float()
        dmo = torch.empty_like(mo)
        _lib.check(_lib.lib().sd_mahalanobis_loss_backward(mo.data_ptr(), tg.data_ptr(), Sc.data_ptr(), tc.data_ptr(),
                                                            Sc.shape[0], dl.data_ptr(), rows, J, F, pred_noise, mse, dmo.data_ptr(),
                                                            _stream(mo.device)))
        need_mo, need_tg = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        return (dmo if need_mo else None), (-dmo if need_tg else None), None, None, None, None


def mahalanobis_loss(model_out: torch.Tensor, target: torch.Tensor, S: torch.Tensor, t: torch.Tensor,
                     pred_noise: bool, mse: bool) -> torch.Tensor:
    """HIP per-row Mahalanobis loss under autograd: model_out / target (rows, J, F) fp32 on the
    device, S (T, J, J), t (rows,) timesteps; J <= 64, F <= 256."""
    if (not model_out.is_cuda or model_out.dtype != torch.float32 or model_out.dim() != 3
            or model_out.shape[1] > MAX_NODES or model_out.shape[2] > 256 or S.dtype != torch.float32):
        raise ValueError("mahalanobis_loss: the HIP training path needs (rows, J <= 64, F <= 256) fp32 device tensors")
    return MahalanobisLossFunction.apply(model_out, target, S, t, pred_noise, mse)


# ---- best-of-k training relaxation (reference src/core/trainer.py:182-222) -----

class BestOfKFunction(torch.autograd.Function):
    """Per sequence the sample whose similarity is smallest and the diffusion loss there:
    `loss_similarity.view(b, -1).min(axis=-1).indices` + `torch.gather` of get_ksimilarity_loss
    (trainer.py:207-222), forward and backward on HIP (`sd_best_of_k` / `_backward`).  The
    similarity carries no gradient (the reference computes it under no_grad)."""

    @staticmethod
    def forward(ctx, loss, sim, k: int):
        lv = loss.contiguous().view(-1)
        nseq = lv.numel() // k
        sv = None if sim is None else sim.detach().contiguous().float().view(-1)
        idx = torch.empty(nseq, device=lv.device, dtype=torch.int64)
        sel = torch.empty(nseq, device=lv.device, dtype=torch.float32)
        _lib.check(_lib.lib().sd_best_of_k(None if sv is None else sv.data_ptr(), lv.data_ptr(), nseq, k,
                                           idx.data_ptr(), sel.data_ptr(), _stream(lv.device)))
        ctx.save_for_backward(idx)
        ctx.k = k
        ctx.mark_non_differentiable(idx)
        return sel, idx

    @staticmethod
    def backward(ctx, dsel, _didx):
        (idx,) = ctx.saved_tensors
        k = ctx.k
        nseq = idx.numel()
        dl = torch.empty(nseq * k, device=idx.device, dtype=torch.float32)
        ds = dsel.contiguous().float()
        _lib.check(_lib.lib().sd_best_of_k_backward(ds.data_ptr(), idx.data_ptr(), nseq, k, dl.data_ptr(),
                                                    _stream(idx.device)))
        return dl, None, None


def best_of_k(loss: torch.Tensor, k: int, sim: Optional[torch.Tensor] = None):
    """(nseq * k,) per-sample diffusion losses (sequence-major: p_losses' repeat_interleave order,
    base.py:264-268) -> (selected loss (nseq,), index (nseq,)): the sample with the smallest `sim`
    (nseq * k values; default the loss itself: the latent space) per sequence, as
    get_ksimilarity_loss (trainer.py:207-222)."""
    if not loss.is_cuda or loss.dtype != torch.float32 or loss.numel() % k or k < 1:
        raise ValueError("best_of_k: an fp32 device tensor of nseq * k losses is required")
    if sim is not None and (sim.numel() != loss.numel() or sim.device != loss.device):
        raise ValueError("best_of_k: sim must hold one value per loss, on the same device")
    return BestOfKFunction.apply(loss, sim, int(k))


def q_sample_groups(x0: torch.Tensor, t: torch.Tensor, sqrt_alphas_cumprod: torch.Tensor, k: int,
                    M: Optional[torch.Tensor] = None, sqrt_one_minus_alphas_cumprod: Optional[torch.Tensor] = None,
                    sel: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed: int = 0,
                    step: int = 0, row0: int = 0, return_noise: bool = False):
    """The forward process for k copies of each of the nseq sequences on HIP (`sd_q_sample_groups`),
    no grad: x0 (nseq, J, D), t (nseq,) and either M (T, J, J) = Umm_sqrt_Lambda_bar_t or
    sqrt_one_minus_alphas_cumprod (T,) -> x_t (nseq * k, J, D) in repeat_interleave order, or with
    `sel` (nseq,) the copy sel[s] of each sequence, (nseq, J, D), bit for bit those rows of the full
    launch.  The noise is `noise` (nseq * k, J, D) when given, else the device Philox stream keyed
    (seed, step, row0 + row); `return_noise` also returns the noise of the rows written."""
    if not x0.is_cuda or x0.dtype != torch.float32 or x0.dim() != 3:
        raise ValueError("q_sample_groups: x0 must be a (nseq, J, D) fp32 device tensor")
    nseq, J, D = x0.shape
    dev = x0.device

    def table(v, name, shape):
        if v.dtype != torch.float32 or v.device != dev or v.dim() != 1 + len(shape) or tuple(v.shape[1:]) != shape:
            raise ValueError(f"q_sample_groups: {name} must be a {('T',) + shape} fp32 tensor on x0's device")
        return v.detach().contiguous()

    ac = table(sqrt_alphas_cumprod, "sqrt_alphas_cumprod", ())
    T = int(ac.shape[0])
    Mc = None if M is None else table(M, "M", (J, J))
    bc = None if sqrt_one_minus_alphas_cumprod is None else table(sqrt_one_minus_alphas_cumprod,
                                                                  "sqrt_one_minus_alphas_cumprod", ())
    for v, name in ((Mc, "M"), (bc, "sqrt_one_minus_alphas_cumprod")):
        if v is not None and v.shape[0] != T:
            raise ValueError(f"q_sample_groups: {name} must hold T = {T} timesteps")
    if t.numel() != nseq:
        raise ValueError(f"q_sample_groups: t must hold one timestep per sequence ({nseq})")
    tc = t.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    sc = None
    if sel is not None:
        if sel.numel() != nseq:
            raise ValueError(f"q_sample_groups: sel must hold one index per sequence ({nseq})")
        sc = sel.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    nc = None
    if noise is not None:
        if tuple(noise.shape) != (nseq * k, J, D) or noise.dtype != torch.float32 or noise.device != dev:
            raise ValueError(f"q_sample_groups: noise must be a ({nseq * k}, {J}, {D}) fp32 tensor on x0's device, "
                             f"got {tuple(noise.shape)}")
        nc = noise.detach().contiguous()
    rows = nseq if sc is not None else nseq * k
    xc = x0.detach().contiguous()
    x_t = torch.empty(rows, J, D, device=dev, dtype=torch.float32)
    eps = torch.empty_like(x_t) if return_noise else None
    _lib.check(_lib.lib().sd_q_sample_groups(
        xc.data_ptr(), tc.data_ptr(), ac.data_ptr(), _lib.ptr(Mc), _lib.ptr(bc), T, nseq, int(k), J, D, _lib.ptr(sc),
        _lib.ptr(nc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(row0), x_t.data_ptr(), _lib.ptr(eps), _stream(dev)))
    return (x_t, eps) if return_noise else x_t


def pose_loss(pred: torch.Tensor, target: torch.Tensor, mse: bool) -> torch.Tensor:
    """AutoEncoder.loss(pred, target, reduction='none') (autoencoder.py:80-98) on HIP (`sd_pose_loss`),
    no grad: pred (nseq, S, T, J, C), target (nseq, T, J, C) -> (nseq, S)."""
    if not pred.is_cuda or pred.dim() != 5 or target.dim() != 4 or pred.shape[0] != target.shape[0] or \
            tuple(pred.shape[2:]) != tuple(target.shape[1:]):
        raise ValueError("pose_loss: pred (nseq, S, T, J, C) and target (nseq, T, J, C) device tensors")
    nseq, S, T, J, C = pred.shape
    p = pred.detach().contiguous().float()
    tg = target.detach().contiguous().float()
    out = torch.empty((nseq, S), device=pred.device, dtype=torch.float32)
    _lib.check(_lib.lib().sd_pose_loss(p.data_ptr(), tg.data_ptr(), nseq, S, T, J, C, int(bool(mse)), out.data_ptr(),
                                       _stream(pred.device)))
    return out
