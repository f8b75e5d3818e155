"""Mirror of the reference's motion autoencoder (SURVEY.md §8f "next" #1): the graph-GRU
`Encoder` that turns the observed past into the conditioning latent, and the `Decoder` that
unrolls the sampled latent into `ph` future frames (`src/core/network/nn/{autoencoder,encoder,
decoder}.py`, `src/core/network/layers/recurrent.py:208-401`).  Same constructor kwargs and
state_dict keys as the reference, so its autoencoder checkpoints load strictly.

`AutoEncoder.decode` -- the step after `sample()` in the evaluation (`eval_prepare_model.py:
106-116`), run on bs x 50 rows for ph frames -- goes to the HIP decoder (`sd_gru_decode`) and
`get_past_embedding` (the conditioning latents) to the HIP encoder (`sd_gru_encode`) when the
module lives on a ROCm device; on the CPU they raise (no CPU evaluation path).  `forward` /
`autoencode` (stage-1 training, autograd) run each GRU as one HIP sequence call per forward
(`training.graph_gru` / `gx_table`) on a ROCm device and stay torch ops on the CPU.

`recurrent_arch_enc` / `recurrent_arch_decoder` also take `StaticGraphLSTM` (`recurrent.py:13-203`,
`encoder.py:55-75`, `decoder.py:47-52,75-78`): the cell keeps a cell state beside `h`, the module an
`initial_hidden_c` layer.  Its sequences run on `training.graph_lstm` under the same conditions
(DESIGN.md §4r2); `decode` / `get_past_embedding` of an LSTM side run the module's forward under
`no_grad` (the HIP sequence forward on a ROCm device, torch ops on the CPU).
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import Parameter

from ... import training as _training
from .layers import StaticGraphLinear

__all__ = ["StaticGraphGRUCell", "StaticGraphGRU", "StaticGraphLSTMCell", "StaticGraphLSTM", "Encoder", "Decoder",
           "AutoEncoder"]


def _gmm(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """graph_structural.py:7-8: per-node x[b, n] @ w[n] (w: (n, in, out))."""
    return torch.einsum("ndo,bnd->bno", w, x)


class StaticGraphGRUCell(nn.Module):
    """recurrent.py:208-366 (the GRU cell; clockwork off -> the update mask is 1)."""

    GATES = 3  # gate blocks stacked in weight_ih / weight_hh / the biases

    def __init__(self, input_size: int, hidden_size: int, num_nodes: Optional[int] = None, dropout: float = 0.,
                 recurrent_dropout: float = 0., graph_influence=None, learn_influence: bool = False,
                 additive_graph_influence=None, learn_additive_graph_influence: bool = False,
                 node_types: Optional[torch.Tensor] = None, weights_per_type: bool = False,
                 clockwork: bool = False, bias: bool = True):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.learn_influence = learn_influence
        self.learn_additive_graph_influence = learn_additive_graph_influence
        if graph_influence is not None:
            num_nodes = graph_influence.shape[0]
            if isinstance(graph_influence, Parameter) or learn_influence:
                self.G = graph_influence if isinstance(graph_influence, Parameter) else Parameter(graph_influence)
            else:
                self.register_buffer("G", graph_influence)
        else:
            assert num_nodes, "Number of Nodes or Graph Influence Matrix has to be given."
            eye = torch.eye(num_nodes, num_nodes)
            if learn_influence:
                self.G = Parameter(eye)
            else:
                self.register_buffer("G", eye)
        if additive_graph_influence is not None:
            if isinstance(additive_graph_influence, Parameter) or learn_additive_graph_influence:
                self.G_add = (additive_graph_influence if isinstance(additive_graph_influence, Parameter)
                              else Parameter(additive_graph_influence))
            else:
                self.register_buffer("G_add", additive_graph_influence)
        elif learn_additive_graph_influence:
            self.G_add = Parameter(torch.zeros_like(self.G))
        else:
            self.G_add = 0.
        if weights_per_type and node_types is None:
            node_types = torch.arange(num_nodes)
        if node_types is not None:
            node_types = torch.as_tensor(node_types, dtype=torch.long)
            nt = int(node_types.max()) + 1
            self.weight_ih = Parameter(torch.empty(nt, self.GATES * hidden_size, input_size))
            self.weight_hh = Parameter(torch.empty(nt, self.GATES * hidden_size, hidden_size))
            self.register_buffer("node_type_index", node_types)
            lead = (nt,)
        else:
            self.weight_ih = Parameter(torch.empty(self.GATES * hidden_size, input_size))
            self.weight_hh = Parameter(torch.empty(self.GATES * hidden_size, hidden_size))
            self.register_buffer("node_type_index", None)
            lead = ()
        if bias:
            self.bias_ih = Parameter(torch.empty(*lead, self.GATES * hidden_size))
            self.bias_hh = Parameter(torch.empty(*lead, self.GATES * hidden_size))
        else:
            self.bias_ih = self.bias_hh = None
        self.clockwork = clockwork
        if clockwork:
            phase = torch.arange(0., hidden_size)
            phase = torch.floor((phase - phase.min()) / phase.max() * 8. + 1.)
        else:
            phase = torch.ones(hidden_size)
        self.register_buffer("phase", phase)
        self.dropout = nn.Dropout(dropout)
        self.r_dropout = nn.Dropout(recurrent_dropout)
        self.num_nodes = num_nodes
        self.init_weights()

    def init_weights(self):
        stdv = 1.0 / math.sqrt(self.hidden_size)  # recurrent.py:310-318
        for w in self.parameters():
            if w is self.G or w is self.G_add:
                continue
            w.data.uniform_(-stdv, stdv)

    def _typed(self, w):
        return w[self.node_type_index] if self.node_type_index is not None else w

    def forward(self, input: torch.Tensor, state, t: int = 0):
        hx, gx = state
        if hx is None:
            hx = input.new_zeros(input.shape[0], self.num_nodes, self.hidden_size)
        if gx is None:
            gx = F.normalize(self.G, p=1., dim=1) if self.learn_influence else self.G
        hx = self.r_dropout(hx)
        w_ih, w_hh = self._typed(self.weight_ih), self._typed(self.weight_hh)
        b_ih = self._typed(self.bias_ih) if self.bias_ih is not None else 0.
        b_hh = self._typed(self.bias_hh) if self.bias_hh is not None else 0.
        mm = _gmm if self.node_type_index is not None else torch.matmul
        c_mask = (torch.remainder(torch.tensor(t + 1., device=input.device), self.phase) < 0.01).type_as(hx)
        x_res = torch.matmul(gx, self.dropout(mm(input, w_ih.transpose(-2, -1))) + b_ih)
        h_res = torch.matmul(gx, mm(hx, w_hh.transpose(-2, -1)) + b_hh)
        i_r, i_z, i_n = x_res.chunk(3, 2)
        h_r, h_z, h_n = h_res.chunk(3, 2)
        r = torch.sigmoid(i_r + h_r)
        z = torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        hy = n - n * z + z * hx
        hy = c_mask * hy + (1 - c_mask) * hx
        gx = gx + self.G_add
        if self.learn_influence or self.learn_additive_graph_influence:
            gx = F.normalize(gx, p=1., dim=1)
        return hy, (hy, gx)


class StaticGraphGRU(nn.Module):
    """recurrent.py:369-391: stacked cells over the time axis of (B, T, N, D) inputs."""

    CELL = StaticGraphGRUCell
    EMPTY_STATE = (None, None)

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, layer_dropout: float = 0.0, **kwargs):
        super().__init__()
        self.layers = nn.ModuleList([self.CELL(input_size, hidden_size, **kwargs)] +
                                    [self.CELL(hidden_size, hidden_size, **kwargs)
                                     for _ in range(num_layers - 1)])
        self.dropout = nn.Dropout(layer_dropout)

    def forward(self, input: torch.Tensor, states: Optional[List] = None, t_i: int = 0):
        if states is None:
            states = [self.EMPTY_STATE] * len(self.layers)
        output_states = []
        output = input
        for i, layer in enumerate(self.layers):
            state = states[i]
            outs = []
            for t, x in enumerate(output.unbind(1)):
                out, state = layer(x, state, t_i + t)
                outs.append(out)
            output = self.dropout(torch.stack(outs, dim=1))
            output_states.append(state)
        return output, output_states


class StaticGraphLSTMCell(StaticGraphGRUCell):
    """recurrent.py:13-167 (the LSTM cell; clockwork off -> the update mask is 1).  Same constructor
    and parameters as the GRU cell with four gate blocks i | f | g | o; `bias_ih` is a parameter
    and a state-dict key that the forward never reads, as in the reference."""

    GATES = 4

    def init_weights(self):
        stdv = 1.0 / math.sqrt(self.hidden_size)  # recurrent.py:115-124
        for w in self.parameters():
            if w is self.G or w is self.G_add:
                continue
            w.data.uniform_(-stdv, stdv)
            if w is self.weight_hh or (w is self.weight_ih and self.weight_ih.dim() == 3):
                w.data[1:] = w.data[0]

    def forward(self, input: torch.Tensor, state, t: int = 0):
        hx, cx, gx = state
        if hx is None:
            hx = input.new_zeros(input.shape[0], self.num_nodes, self.hidden_size)
        if cx is None:
            cx = input.new_zeros(input.shape[0], self.num_nodes, self.hidden_size)
        if gx is None:
            gx = F.normalize(self.G, p=1., dim=1) if self.learn_influence else self.G
        hx = self.r_dropout(hx)
        w_ih, w_hh = self._typed(self.weight_ih), self._typed(self.weight_hh)
        b_hh = self._typed(self.bias_hh) if self.bias_hh is not None else 0.
        mm = _gmm if self.node_type_index is not None else torch.matmul
        c_mask = (torch.remainder(torch.tensor(t + 1., device=input.device), self.phase) < 0.01).type_as(cx)
        gates = self.dropout(mm(input, w_ih.transpose(-2, -1))) + mm(hx, w_hh.transpose(-2, -1)) + b_hh
        i, f, g, o = torch.matmul(gx, gates).chunk(4, 2)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        cy = c_mask * (f * cx + i * g) + (1 - c_mask) * cx
        hy = o * torch.tanh(cy)
        gx = gx + self.G_add
        if self.learn_influence or self.learn_additive_graph_influence:
            gx = F.normalize(gx, p=1., dim=1)
        return hy, (hy, cy, gx)


class StaticGraphLSTM(StaticGraphGRU):
    """recurrent.py:170-196: stacked LSTM cells over the time axis; states are (h, s, gx)."""

    CELL = StaticGraphLSTMCell
    EMPTY_STATE = (None, None, None)


def _no_dropout(*mods) -> bool:
    return all(m.p == 0.0 or not m.training for m in mods)


def _hip_sequence_ok(rnn: "StaticGraphGRU", x: torch.Tensor, *dropouts) -> bool:
    """Whether a GRU forward takes the HIP sequence path (training.graph_gru): fp32 tensors on a
    ROCm device, the HIP training switch on, one layer, clockwork off, no active dropout, and a
    cell the kernels cover.  Otherwise the torch ops below run, unchanged."""
    if not (x.is_cuda and x.dtype == torch.float32 and _training.hip_training_enabled() and len(rnn.layers) == 1):
        return False
    cell = rnn.layers[0]
    if cell.clockwork or not _no_dropout(cell.dropout, cell.r_dropout, rnn.dropout, *dropouts):
        return False
    H, J = cell.hidden_size, cell.num_nodes
    if cell.weight_hh.dtype != torch.float32 or H % 16 or H > _training.GRU_MAX_HIDDEN or not 1 <= J <= _training.MAX_NODES:
        return False
    if x.shape[-2] != J:
        return False
    # a fixed additive matrix without re-normalisation (gx_t = G + t G_add) is not built
    return not (isinstance(cell.G_add, torch.Tensor) and not (cell.learn_influence or cell.learn_additive_graph_influence))


def _hip_linear(mod: StaticGraphLinear, x: torch.Tensor) -> torch.Tensor:
    """A StaticGraphLinear through GraphLinearFunction whether or not grad is enabled (under
    no_grad the same HIP forward runs and keeps nothing)."""
    g = mod.ghat()
    if mod.weight.dtype != torch.float32 or not mod._hip_ok(x, g):
        return mod(x)
    return _training.graph_linear(x, mod.weight, mod.bias, g, mod._node_types_on(x.device))


def _hip_gru_sequence(cell: StaticGraphGRUCell, x: torch.Tensor, h0: torch.Tensor, steps: int):
    """The cell over `steps` steps on HIP: x (B, Ta, J, D) with Ta = steps or 1 (the same input
    at every step) -> hs (B, steps, J, H) and the mixing matrix after the last step."""
    J = cell.num_nodes
    dev = x.device
    eye = getattr(cell, "_eye", None)
    if eye is None or eye.device != dev:
        eye = cell._eye = torch.eye(J, device=dev, dtype=torch.float32)
    nt = cell.node_type_index
    # unmixed input projections W_ih x + b_ih over all B Ta rows (identity mixing matrix)
    a = _training.graph_linear(x, cell.weight_ih, cell.bias_ih, eye, nt)
    gx, gx_last = _hip_gx(cell, steps)
    hs = _training.graph_gru(a, h0, gx, cell.weight_hh, cell.bias_hh, nt, steps=steps)
    return hs, gx_last


def _hip_gx(cell: StaticGraphGRUCell, steps: int):
    """The cell's mixing matrices of `steps` steps, (Tg, J, J) with Tg = steps or 1, and the matrix
    after the last step."""
    if isinstance(cell.G_add, torch.Tensor):
        table = _training.gx_table(cell.G, cell.G_add, steps + 1, normalize0=cell.learn_influence)
        gx, gx_last = table[:steps], table[steps]
    else:  # gx never changes: re-normalising an L1-normalised matrix is the identity
        if not cell.learn_influence:
            gx_last = cell.G
        elif _training.hip_gate():
            gx_last = _training.l1norm_rows(cell.G, 1e-12)
        else:
            gx_last = F.normalize(cell.G, p=1., dim=1)
        gx = gx_last.unsqueeze(0)
    return gx, gx_last


def _hip_lstm_sequence(cell: "StaticGraphLSTMCell", x: torch.Tensor, h0: torch.Tensor, s0: torch.Tensor, steps: int):
    """The LSTM cell over `steps` steps on HIP (training.graph_lstm): x (B, Ta, J, D)
    with Ta = steps or 1 -> hs (B, steps, J, H), the cell state and the mixing matrix after the
    last step."""
    dev = x.device
    eye = getattr(cell, "_eye", None)
    if eye is None or eye.device != dev:
        eye = cell._eye = torch.eye(cell.num_nodes, device=dev, dtype=torch.float32)
    nt = cell.node_type_index
    # unmixed input projections W_ih x over all B Ta rows (identity mixing matrix; bias_ih is unused)
    a = _training.graph_linear(x, cell.weight_ih, None, eye, nt)
    gx, gx_last = _hip_gx(cell, steps)
    hs, s_last = _training.graph_lstm(a, h0, s0, gx, cell.weight_hh, cell.bias_hh, nt, steps=steps)
    return hs, s_last, gx_last


_RECURRENT = {"StaticGraphGRU": StaticGraphGRU, "StaticGraphLSTM": StaticGraphLSTM}


def _recurrent(arch: str):
    if arch not in _RECURRENT:
        raise NotImplementedError(f"recurrent arch {arch!r}: only StaticGraphGRU (the released configs) and "
                                  "StaticGraphLSTM are built")
    return _RECURRENT[arch]


def _is_lstm(arch: str) -> bool:
    return arch == "StaticGraphLSTM"


class Encoder(nn.Module):
    """encoder.py:10-81: GRU over the observed frames, then tanh(fc(last hidden))."""

    def __init__(self, num_nodes: int, input_size: int, hidden_size: int, output_size: int,
                 node_types: Optional[torch.Tensor] = None, enc_num_layers: int = 1, dropout: float = 0.,
                 encoder_act: str = "tanh", recurrent_arch: str = "StaticGraphGRU", **kwargs):
        super().__init__()
        assert encoder_act in ("tanh", "identity"), "not implemented"
        self.activation_fn = nn.Tanh() if encoder_act == "tanh" else nn.Identity()
        self.num_layers = enc_num_layers
        self.recurrent_arch = recurrent_arch
        self.rnn = _recurrent(recurrent_arch)(input_size, hidden_size, num_layers=enc_num_layers,
                                              node_types=node_types, num_nodes=num_nodes, bias=True,
                                              clockwork=False, learn_influence=True)
        self.fc = StaticGraphLinear(hidden_size, output_size, num_nodes=num_nodes, node_types=node_types,
                                    bias=True, learn_influence=True)
        self.initial_hidden1 = StaticGraphLinear(input_size, hidden_size, num_nodes=num_nodes,
                                                 node_types=node_types, bias=True, learn_influence=True)
        if _is_lstm(recurrent_arch):  # encoder.py:55-61
            self.initial_hidden_c = StaticGraphLinear(input_size, hidden_size, num_nodes=num_nodes,
                                                      node_types=node_types, bias=True, learn_influence=True)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor, state=None):
        hip = state is None and x.dim() == 4 and x.shape[1] >= 1 and _hip_sequence_ok(self.rnn, x, self.dropout)
        if _is_lstm(self.recurrent_arch):
            if hip:  # the whole sequence in one HIP call (forward + BPTT)
                hs, s_last, gx = _hip_lstm_sequence(self.rnn.layers[0], x, _hip_linear(self.initial_hidden1, x[:, 0]),
                                                    _hip_linear(self.initial_hidden_c, x[:, 0]), x.shape[1])
                h_last = hs[:, -1]
                return self.activation_fn(_hip_linear(self.fc, h_last)), [(h_last, s_last, gx)]
            if state is None:  # encoder.py:64-75
                state = [(self.initial_hidden1(x[:, 0]), self.initial_hidden_c(x[:, 0]), None)] * self.num_layers
            y, state = self.rnn(input=x, states=state)
            return self.activation_fn(self.fc(self.dropout(y[:, -1]))), state
        if hip:
            # the whole sequence in one HIP call (forward + BPTT)
            hs, gx = _hip_gru_sequence(self.rnn.layers[0], x, _hip_linear(self.initial_hidden1, x[:, 0]), x.shape[1])
            h_last = hs[:, -1]
            return self.activation_fn(_hip_linear(self.fc, h_last)), [(h_last, gx)]
        if state is None:
            state = [(self.initial_hidden1(x[:, 0]), None)] * self.num_layers
        y, state = self.rnn(input=x, states=state)
        return self.activation_fn(self.fc(self.dropout(y[:, -1]))), state


class Decoder(nn.Module):
    """decoder.py:9-104: GRU unrolled for ph frames from [last frame, latent], tanh(fc(h))."""

    def __init__(self, num_nodes: int, feature_size: int, input_size: int, hidden_size: int, output_size: int,
                 node_types: Optional[torch.Tensor] = None, dec_num_layers: int = 1, dropout: float = 0.,
                 param_groups=None, recurrent_arch_decoder: str = "StaticGraphGRU", **kwargs):
        super().__init__()
        self.param_groups = param_groups
        self.num_layers = dec_num_layers
        self.if_consider_hip = kwargs["if_consider_hip"]
        self.activation_fn = nn.Tanh()
        self.recurrent_arch = recurrent_arch_decoder
        self.rnn = _recurrent(recurrent_arch_decoder)(feature_size + input_size, hidden_size, num_nodes=num_nodes,
                                                      num_layers=dec_num_layers, learn_influence=True,
                                                      node_types=node_types, recurrent_dropout=dropout,
                                                      learn_additive_graph_influence=True, clockwork=False)
        self.initial_hidden_h = StaticGraphLinear(feature_size + input_size, hidden_size, num_nodes=num_nodes,
                                                  learn_influence=True, node_types=node_types)
        if _is_lstm(recurrent_arch_decoder):  # decoder.py:47-52
            self.initial_hidden_c = StaticGraphLinear(feature_size + input_size, hidden_size, num_nodes=num_nodes,
                                                      learn_influence=True, node_types=node_types)
        self.fc = StaticGraphLinear(hidden_size, output_size, num_nodes=num_nodes, learn_influence=True,
                                    node_types=node_types)
        self.dropout = nn.Dropout(dropout)

    def init_recurrent_hidden(self, x, h, z, state=None):
        x_t = x[:, -1]
        x_t_1 = x[:, -2] if state is None else state
        init = torch.cat([x_t_1, h], dim=-1)
        rnn_h = self.initial_hidden_h(init)
        if _is_lstm(self.recurrent_arch):  # decoder.py:75-78
            hidden = [(rnn_h, self.initial_hidden_c(init), None)] * self.num_layers
        else:
            hidden = [(rnn_h, None)] * self.num_layers
        return torch.cat([x_t, h], dim=-1).unsqueeze(1), hidden

    def forward(self, x: torch.Tensor, h: torch.Tensor, z: torch.Tensor, ph: int = 1, state=None):
        """Training forward (autograd): one HIP sequence call on a ROCm device, torch ops
        otherwise; `AutoEncoder.decode` uses the HIP decoder."""
        x_t_s = x[:, -1].clone()
        if ph >= 1 and _hip_sequence_ok(self.rnn, x, self.dropout):
            x_t_1 = x[:, -2] if state is None else state
            init = torch.cat([x_t_1, h], dim=-1)
            rnn_h = _hip_linear(self.initial_hidden_h, init)
            rec_input = torch.cat([x[:, -1], h], dim=-1).unsqueeze(1)  # the same input at every step
            if _is_lstm(self.recurrent_arch):
                hs = _hip_lstm_sequence(self.rnn.layers[0], rec_input, rnn_h, _hip_linear(self.initial_hidden_c, init),
                                        ph)[0]
            else:
                hs, _ = _hip_gru_sequence(self.rnn.layers[0], rec_input, rnn_h, ph)
            return self.activation_fn(_hip_linear(self.fc, hs)), x_t_s  # fc over all ph states at once
        rec_input, hidden = self.init_recurrent_hidden(x=x, h=h, z=z, state=state)
        out = []
        for i in range(ph):
            rnn_out, hidden = self.rnn(input=rec_input, states=hidden, t_i=i)
            out.append(self.activation_fn(self.fc(self.dropout(rnn_out.squeeze(1)))))
        return torch.stack(out, dim=1), x_t_s


class AutoEncoder(nn.Module):
    """autoencoder.py:8-102."""

    def __init__(self, num_nodes: int, encoder_hidden_size: int, decoder_hidden_size: int, latent_size: int,
                 node_types: Optional[torch.Tensor] = None, input_size: int = 3, z_activation: str = "tanh",
                 enc_num_layers: int = 1, loss_pose_type: str = "l1", **kwargs):
        super().__init__()
        self.param_groups = [{}]
        self.latent_size = latent_size
        self.loss_pose_type = loss_pose_type
        self.encoder = Encoder(num_nodes=num_nodes, input_size=input_size, hidden_size=encoder_hidden_size,
                               output_size=latent_size, node_types=node_types, enc_num_layers=enc_num_layers,
                               recurrent_arch=kwargs["recurrent_arch_enc"])
        assert kwargs["output_size"] == input_size
        self.decoder = Decoder(num_nodes=num_nodes, input_size=latent_size, feature_size=input_size,
                               hidden_size=decoder_hidden_size, node_types=node_types,
                               param_groups=self.param_groups, **kwargs)
        assert z_activation in ["tanh", "identity"], \
            f"z_activation must be either 'tanh' or 'identity', but got {z_activation}"
        self.z_activation = nn.Tanh() if z_activation == "tanh" else nn.Identity()
        self._engine = None

    def forward(self, x):
        h, _ = self.encoder(x)
        return h

    def _hip(self):
        from ... import decoder_engine

        if self._engine is None:
            self._engine = decoder_engine.DecoderEngine(self.decoder, self.encoder,
                                                        z_tanh=isinstance(self.z_activation, nn.Tanh))
        return self._engine

    def get_past_embedding(self, past, state=None):
        """z_activation(encoder(past)) on the HIP encoder (the conditioning latents of sample(),
        eval_prepare_model.py:89-99); no_grad as the reference."""
        if state is not None:
            raise NotImplementedError("get_past_embedding(state=...) is not used by the evaluation and not built")
        if _is_lstm(self.encoder.recurrent_arch):
            # no LSTM engine: the module's own forward under no_grad (the HIP sequence forward on a
            # ROCm device, torch ops on the CPU)
            with torch.no_grad():
                return self.z_activation(self(past))
        return self._hip().encode(past)

    def get_embedding(self, future, state=None):
        return self.forward(future)

    def get_train_embeddings(self, y, past, state=None):
        return self.get_past_embedding(past, state=state), self.get_embedding(y, state=state)

    def decode(self, x: torch.Tensor, h: torch.Tensor, z: torch.Tensor, ph: int = 1, state=None):
        """(B, T_obs, J, F) past, (B, J, latent) sampled latent -> (B, ph, J, F) on the HIP decoder
        (decoder.py:85-104 semantics; `z` is unused there too)."""
        if state is not None:
            raise NotImplementedError("decode(state=...) is not used by the evaluation and not built")
        if _is_lstm(self.decoder.recurrent_arch):
            with torch.no_grad():
                return self.decoder(x=x[:, -2:], h=h, z=z, ph=ph)[0]
        return self._hip().decode(x[:, -2:], h, ph)

    def autoencode(self, y, past, ph=1, state=None):
        """Training-time reconstruction (autograd): HIP sequence calls on a ROCm device, torch
        ops on the CPU."""
        with torch.no_grad():
            z_past = self.z_activation(self(past))
        z = self.get_embedding(y, state=state)
        out, _ = self.decoder(x=past[:, -2:], h=z, z=z_past, ph=ph, state=state)
        return out, z_past, z

    def loss(self, y_pred, y, type=None, reduction="mean", **kwargs):
        type = self.loss_pose_type if type is None else type
        if type == "mse":
            out = nn.MSELoss(reduction="none")(y_pred, y)
        elif type in ["l1", "L1"]:
            out = nn.L1Loss(reduction="none")(y_pred, y)
        else:
            assert 0, "Not implemnted"
        loss = out.sum(-1).mean(-1).mean(-1)
        if reduction == "mean":
            return loss.mean()
        if reduction == "none":
            return loss
        assert 0, "Not implemnted"
