"""The optimizer tail of a training step on the HIP engine: gradient-norm clipping,
the Adam / AdamW update and the EMA of the weights, each as one multi-tensor launch per 40 tensors
(csrc/sd_optim.hip) instead of a string of torch launches.

`FusedAdam` replaces `clip_grad_norm_` + `torch.optim.Adam` / `AdamW` (reference
src/core/trainer.py:33, :93-95, :153, :267-275); `EMA` replaces `ema_pytorch.EMA` (:159, :275).
Both keep the state layout of what they replace, so checkpoints move either way.  Neither ever
synchronises with the device: the gradient norm stays a device scalar.

There is no CPU path: constructing, `state_dict()` and `load_state_dict()` work anywhere, but
`FusedAdam.step()` and `EMA.update()` raise `SkelDiffError` unless every tensor is a contiguous fp32
tensor on one ROCm device.
"""
from __future__ import annotations

import copy
import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import SkelDiffError, check

_PARAM_DT = np.dtype([("p", "u8"), ("grad", "u8"), ("exp_avg", "u8"), ("exp_avg_sq", "u8"), ("max_exp_avg_sq", "u8"),
                      ("numel", "i8"), ("step", "i8"), ("lr", "f8"), ("weight_decay", "f8")])
assert _PARAM_DT.itemsize == ctypes.sizeof(_lib.SDOptimParam)


def _check_tensors(who: str, named) -> torch.device:
    """Every tensor a contiguous fp32 tensor on one ROCm device, or SkelDiffError naming the first that is not."""
    dev = None
    for name, t in named:
        if t.device.type != "cuda":
            raise SkelDiffError(f"{who} runs on the HIP engine only: {name} is on {t.device}, not on a ROCm device")
        if t.dtype != torch.float32:
            raise SkelDiffError(f"{who} runs on the HIP engine only: {name} is {t.dtype}, not torch.float32")
        if t.layout != torch.strided or not t.is_contiguous():
            raise SkelDiffError(f"{who} runs on the HIP engine only: {name} is not contiguous")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise SkelDiffError(f"{who} runs on the HIP engine only: {name} is on {t.device}, other tensors on {dev} "
                                "(one optimizer per device)")
    return dev


def _u8(ptrs) -> np.ndarray:
    return np.asarray(ptrs, dtype=np.uint64)


class FusedAdam(torch.optim.Optimizer):
    """Adam / AdamW with gradient-norm clipping folded in, on the HIP engine.

    Per element, in float32 (`coef` is read from device memory):
        g    <- g * coef                    coef = min(max_grad_norm / (||g||_2 + 1e-6), 1), 1 without clipping
        Adam:  g' = g + wd * p              AdamW (decoupled_weight_decay): p <- p * (1 - lr * wd), g' = g
        m    <- beta1 * m + (1 - beta1) * g'
        v    <- beta2 * v + (1 - beta2) * g'^2
        vmax <- max(vmax, v)                (amsgrad)
        p    <- p - lr / (1 - beta1^t) * m / (sqrt(v or vmax) / sqrt(1 - beta2^t) + eps)
    The norm is over the gradients of all param groups, as `clip_grad_norm_(model.parameters(), ...)`
    computes it (norm_type 2, error_if_nonfinite=False), summed in float64 in a fixed order.

    It is a `torch.optim.Optimizer`: param groups and LR schedulers work, `lr` and `weight_decay` are
    read from the groups at each step, the step count is kept per parameter, and a parameter whose
    `grad is None` is skipped.  The state uses torch's keys (`step`, `exp_avg`, `exp_avg_sq`,
    `max_exp_avg_sq`), so a `torch.optim.Adam` / `AdamW` state dict (the `'opt'` entry of a reference
    checkpoint) loads into it and its own loads into them.

    max_grad_norm: None, or the `max_norm` of the `clip_grad_norm_` call this replaces.
    store_clipped_grads: write the clipped gradients back, so `p.grad` holds what `clip_grad_norm_`
        would have left there (default); False saves that store and leaves the gradients untouched.
    last_grad_norm: after a step with clipping, the total norm BEFORE clipping, a float32 scalar on the
        device (what `clip_grad_norm_` returns).  It is a view of a buffer the next step overwrites.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 decoupled_weight_decay=False, max_grad_norm: Optional[float] = None, store_clipped_grads: bool = True):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a number (it is read on the host at every step)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        # the keys torch.optim.Adam keeps in a group, in its order, so that state dicts interchange
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.store_clipped_grads = bool(store_clipped_grads)
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._norm_coef: Optional[torch.Tensor] = None  # device {total_norm, coef}
        self._workspace: Optional[torch.Tensor] = None
        self._plans = {}       # (ids of the parameters with a gradient) -> _Plan
        # The per-parameter step counts live side by side in one host tensor and state[p]["step"] is
        # a 0-dim view of it: a step advances them with one add, not one per parameter.
        self._step_pool: Optional[torch.Tensor] = None
        self._step_index = {}  # parameter -> its element of the pool

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:  # a group saved by an older torch lacks some keys
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        # also reached through unpickling, which keeps torch's three attributes only
        for name, value in (("max_grad_norm", None), ("store_clipped_grads", True), ("last_grad_norm", None),
                            ("_norm_coef", None), ("_workspace", None)):
            self.__dict__.setdefault(name, value)
        self._plans, self._step_pool, self._step_index = {}, None, {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():  # the step count is read on the host: never from a device tensor
            s = st.get("step")
            if s is None:
                continue
            if not torch.is_tensor(s):
                st["step"] = torch.tensor(float(s), dtype=torch.float32)
            elif s.device.type != "cpu":
                st["step"] = s.detach().cpu()
        self._plans = {}

    def state_dict(self):
        sd = super().state_dict()  # the counts as tensors of their own, as torch saves them
        sd["state"] = {k: dict(v, step=v["step"].clone()) if "step" in v else v for k, v in sd["state"].items()}
        return sd

    def _pool_steps(self, ps, states):
        """Moves the step counts of `ps` into the pool (created, loaded or first seen: a tensor of
        its own); returns their pool indices."""
        total = sum(len(g["params"]) for g in self.param_groups)
        pool = self._step_pool
        if pool is None or pool.numel() < total:
            new = torch.zeros(total, dtype=torch.float32)
            if pool is not None:
                new[:pool.numel()] = pool
            for q, i in self._step_index.items():
                st = self.state.get(q)
                if st is not None and "step" in st and st["step"]._base is pool:
                    st["step"] = new[i]
            self._step_pool = pool = new
            self._plans = {}
        idx = []
        for p, st in zip(ps, states):
            i = self._step_index.setdefault(p, len(self._step_index))
            s = st["step"]
            if s._base is not pool or s.storage_offset() != i:
                pool[i] = float(s)
                st["step"] = pool[i]
            idx.append(i)
        return np.asarray(idx, dtype=np.int64)

    def _init_state(self, p, amsgrad):
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)  # on the host, as torch keeps it
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if amsgrad and "max_exp_avg_sq" not in st:
            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _build_plan(self, ps, gs, counts):
        """The slow path, taken when the set of parameters with a gradient (or their storage) changes:
        checks every tensor by name, creates missing state and fills the table's fixed columns."""
        named, k = [], 0
        for gi, n in enumerate(counts):
            for j in range(n):
                if gs[k].is_sparse:
                    raise SkelDiffError("FusedAdam.step runs on the HIP engine only: sparse gradients are not supported")
                named.append((f"parameter {j} (of those with a gradient) of group {gi}", ps[k]))
                named.append((f"the gradient of parameter {j} (of those with a gradient) of group {gi}", gs[k]))
                k += 1
        plan = _Plan()
        plan.dev = _check_tensors("FusedAdam.step", named)
        plan.ps, plan.pptr = ps, [p.data_ptr() for p in ps]
        plan.tab = np.zeros(len(ps), dtype=_PARAM_DT)
        plan.groups, states, k = [], [], 0
        for group, n in zip(self.param_groups, counts):
            amsgrad = bool(group["amsgrad"])
            if n:
                plan.groups.append((group, k, k + n, amsgrad))
            keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
            for j, p in enumerate(ps[k:k + n]):
                st = self._init_state(p, amsgrad)
                for key in keys:
                    if st[key].numel() != p.numel():
                        raise SkelDiffError(f"FusedAdam.step: state {key!r} of parameter {j} has {st[key].numel()} "
                                            f"elements, the parameter {p.numel()}")
                    plan.tab[key][k + j] = st[key].data_ptr()
                states.append(st)
            _check_tensors("FusedAdam.step", [("a parameter", p) for p in ps[k:k + 1]] + [
                (f"state {key!r} of parameter {j}", st[key]) for j, st in enumerate(states[k:k + n]) for key in keys])
            k += n
        plan.tab["p"] = plan.pptr
        plan.tab["numel"] = [p.numel() for p in ps]
        plan.numel = np.ascontiguousarray(plan.tab["numel"])
        plan.step_idx = self._pool_steps(ps, states)
        plan.step_mask = torch.zeros_like(self._step_pool)
        plan.step_mask[torch.from_numpy(plan.step_idx)] = 1.0
        plan.need = _lib.lib().sd_optim_workspace_bytes(plan.numel.ctypes.data, len(ps))
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps, gs, counts = [], [], []
        for group in self.param_groups:
            if group["maximize"] or group["differentiable"] or group["capturable"]:
                raise SkelDiffError("FusedAdam: maximize, differentiable and capturable are not supported")
            n0 = len(ps)
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    ps.append(p)
                    gs.append(g)
            counts.append(len(ps) - n0)
        if not ps:
            return loss
        # The table's fixed columns are kept per set of parameters with a gradient; a parameter that
        # moved to other storage, or an amsgrad switch, rebuilds them.  The gradients are looked at
        # on every step: their pointers change with zero_grad(set_to_none=True).
        key = tuple(map(id, ps))
        plan = self._plans.get(key)
        if plan is not None and (plan.pptr != [p.data_ptr() for p in ps] or
                                 any(bool(g["amsgrad"]) != a for g, _, _, a in plan.groups)):
            plan = None
        if plan is None:
            plan = self._build_plan(ps, gs, counts)  # (may empty self._plans: a larger step pool)
            if len(self._plans) >= 8:
                self._plans.clear()
            self._plans[key] = plan
        gptr = []
        for g in gs:  # torch keeps a gradient on its parameter's device and in its dtype
            if not g.is_contiguous():
                raise SkelDiffError("FusedAdam.step runs on the HIP engine only: a gradient is not contiguous")
            gptr.append(g.data_ptr())
        tab, dev = plan.tab, plan.dev
        tab["grad"] = gptr
        self._step_pool.add_(plan.step_mask)
        tab["step"] = self._step_pool.numpy()[plan.step_idx]
        L = _lib.lib()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            coef_ptr = None
            if self.max_grad_norm is not None:
                if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < plan.need:
                    self._workspace = torch.empty(max(plan.need, 8), dtype=torch.uint8, device=dev)
                if self._norm_coef is None or self._norm_coef.device != dev:
                    self._norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)
                    self.last_grad_norm = self._norm_coef[0]
                grad_col = np.ascontiguousarray(tab["grad"])
                check(L.sd_optim_grad_norm(grad_col.ctypes.data, plan.numel.ctypes.data, len(ps), float(self.max_grad_norm),
                                           self._norm_coef.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(),
                                           stream))
                coef_ptr = self._norm_coef.data_ptr() + 4
            for group, a, b, amsgrad in plan.groups:
                tab["lr"][a:b] = float(group["lr"])
                tab["weight_decay"][a:b] = float(group["weight_decay"])
                flags = (_lib.SD_OPTIM_AMSGRAD if amsgrad else 0) | \
                        (_lib.SD_OPTIM_DECOUPLED_WD if group["decoupled_weight_decay"] else 0) | \
                        (_lib.SD_OPTIM_STORE_GRADS if coef_ptr is not None and self.store_clipped_grads else 0)
                b1, b2 = group["betas"]
                check(L.sd_optim_adam_step(tab.ctypes.data + a * _PARAM_DT.itemsize, b - a, float(b1), float(b2),
                                           float(group["eps"]), flags, coef_ptr, stream))
        return loss


class _Plan:
    """What FusedAdam.step keeps between steps for one set of parameters with a gradient."""
    __slots__ = ("dev", "ps", "pptr", "tab", "numel", "groups", "step_idx", "step_mask", "need")


class EMA(torch.nn.Module):
    """Exponential moving average of a model's weights on the HIP engine, with the warm-up schedule
    and the state layout of `ema_pytorch.EMA` (reference src/core/trainer.py:159, :275).

    `update()` reads `step`, then increments it, and acts only when the value it read is a multiple
    of `update_every`.  While that value is <= `update_after_step`, or before the first
    initialisation, it copies the model's parameters and buffers into `ema_model`.  Otherwise, with

        e     = max(step_after_increment - update_after_step - 1, 0)
        decay = 0                                                         if e == 0
                clamp(1 - (1 + e / inv_gamma) ** (-power), min_value, beta)   otherwise

    every parameter becomes `lerp(ema, p, 1 - decay)` in one launch per 40 tensors, and the buffers
    are copied (in this model they are schedule and covariance constants, not averaged statistics).

    `ema_pytorch` is not a dependency of this package: the formula above is restated from its
    documented behaviour and NOT pinned against the package (unpinned at the
    third-party boundary).

    state_dict keys: `ema_model.<name>`, `initted`, `step`.  The step count and the initialised flag
    are kept on the host as well, so `update()` never reads a device tensor.
    """

    def __init__(self, model: torch.nn.Module, beta: float = 0.995, update_every: int = 10, update_after_step: int = 100,
                 power: float = 2 / 3, min_value: float = 0.0, inv_gamma: float = 1.0):
        super().__init__()
        if update_every < 1:
            raise ValueError(f"EMA: update_every must be >= 1, got {update_every}")
        self._online = [model]  # in a list: not a submodule, so not part of the state dict
        self.ema_model = copy.deepcopy(model)
        self.ema_model.requires_grad_(False)
        self.beta, self.update_every, self.update_after_step = float(beta), int(update_every), int(update_after_step)
        self.power, self.min_value, self.inv_gamma = float(power), float(min_value), float(inv_gamma)
        self.register_buffer("initted", torch.tensor(False))
        self.register_buffer("step", torch.tensor(0))
        self._step, self._initted = 0, False
        self.register_load_state_dict_post_hook(EMA._after_load)

    @staticmethod
    def _after_load(module, incompatible_keys):
        module._step, module._initted = int(module.step.item()), bool(module.initted.item())

    @property
    def model(self) -> torch.nn.Module:
        return self._online[0]

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)

    def get_current_decay(self) -> float:
        """A pure host function of the step count (see the class docstring)."""
        e = max(self._step - self.update_after_step - 1, 0)
        if e <= 0:
            return 0.0
        value = 1.0 - (1.0 + e / self.inv_gamma) ** (-self.power)
        return min(max(value, self.min_value), self.beta)

    @torch.no_grad()
    def update(self) -> None:
        step = self._step
        pairs = self._pairs()  # refuses CPU tensors before anything changes
        self._step += 1
        self.step += 1
        if step % self.update_every != 0:
            return
        if step <= self.update_after_step or not self._initted:
            self._blend(pairs, 1.0)
            if not self._initted:
                self._initted = True
                self.initted.fill_(True)
            return
        self._blend(pairs, 1.0 - self.get_current_decay())

    def copy_params_from_model_to_ema(self) -> None:
        with torch.no_grad():
            self._blend(self._pairs(), 1.0)

    def _pairs(self):
        ema_p, cur_p = list(self.ema_model.named_parameters()), list(self.model.named_parameters())
        ema_b, cur_b = list(self.ema_model.named_buffers()), list(self.model.named_buffers())
        if [n for n, _ in ema_p] != [n for n, _ in cur_p] or [n for n, _ in ema_b] != [n for n, _ in cur_b]:
            raise SkelDiffError("EMA: the model's parameters or buffers changed since the EMA was built")
        named = [(f"parameter {n}", t) for n, t in cur_p] + [(f"ema_model parameter {n}", t) for n, t in ema_p]
        dev = _check_tensors("EMA.update", named)
        return dev, [(a, p) for (_, a), (_, p) in zip(ema_p, cur_p)], [(a, b) for (_, a), (_, b) in zip(ema_b, cur_b)]

    def _blend(self, pairs, weight: float) -> None:
        dev, params, buffers = pairs
        if params:
            with torch.cuda.device(dev):
                ema = _u8([a.data_ptr() for a, _ in params])
                cur = _u8([p.data_ptr() for _, p in params])
                numel = np.asarray([p.numel() for _, p in params], dtype=np.int64)
                check(_lib.lib().sd_optim_ema_update(ema.ctypes.data, cur.ctypes.data, numel.ctypes.data, len(params),
                                                     float(weight), torch.cuda.current_stream(dev).cuda_stream))
        for a, b in buffers:
            a.copy_(b)
