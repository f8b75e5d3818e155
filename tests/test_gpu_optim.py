"""The fused optimizer step on the device: `optim.FusedAdam` and `optim.EMA` against
torch on the CPU in float64.

Reference: always torch on the CPU in float64 (`clip_grad_norm_` + `torch.optim.Adam` / `AdamW`), fed
the same float32 parameters and gradients; never the code under test.
Yardstick (that of tests/test_gpu_gru_train.py): err = max|x - x64| / max|x64| and
err_hip <= 8 x err_torch32, err_torch32 being the same torch path in float32 on the CPU.  The error is
pooled over all tensors of a case per kind of state (p, exp_avg, exp_avg_sq, max_exp_avg_sq, clipped
grad, EMA weights), so that a one-element tensor cannot make err_torch32 zero by luck; where
err_torch32 is exactly 0, err_hip must be at most 2^-23.
The norm: relative 2^-23 of the float64 norm (exact squares, a float64 sum, one rounding to float32).

Gradient scales cycle 0.1 / 1 / 10 over a base of 3e-3, which puts the total norm of the shapes below
(286,000 elements) near 0.16 / 1.6 / 16: with max_grad_norm = 1 the first step of each cycle does not
clip and the others do."""
import copy
import itertools

import pytest
import torch

from skeletondiffusion_amd import optim, synthetic, training
from skeletondiffusion_amd.skeletons import skeleton

FACTOR = 8.0
EPS23 = 2.0 ** -23
CHUNK = 16384  # sd::optim::kChunk
SHAPES = [(0,), (1,), (3,), (5,), (30,), (21, 21), (4097,), (9, 288, 96), (CHUNK,), (CHUNK + 1,)]
SCALES = (0.1, 1.0, 10.0)
BASE = 3e-3
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
KINDS = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "grad")


def make_inputs(shapes, steps, seed=0, base=BASE):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (base * SCALES[it % 3]) for s in shapes] for it in range(steps)]
    return init, grads


_INPUTS = {}


def inputs(steps=6):
    """One set of parameters and gradients for all cases over SHAPES, made once and never changed."""
    if steps not in _INPUTS:
        _INPUTS[steps] = make_inputs(SHAPES, steps)
    return _INPUTS[steps]


def group_split(ps, grouped):
    if not grouped:
        return [dict(params=ps)]
    return [dict(params=ps[::2], lr=LR, weight_decay=0.01), dict(params=ps[1::2], lr=3 * LR, weight_decay=0.03)]


def run(init, grads, *, hip, dtype=torch.float32, device="cpu", decoupled, amsgrad, wd, max_norm, grouped=False,
        skip=None, store=True, hook=None):
    """`len(grads)` steps; skip = (step index, parameter index) leaves that gradient None.  Returns the
    final state per kind, the clipped gradients of every step, the norms and the optimizer."""
    ps = [torch.nn.Parameter(t.clone().to(device=device, dtype=dtype)) for t in init]
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, amsgrad=amsgrad)
    if hip:
        opt = optim.FusedAdam(group_split(ps, grouped), decoupled_weight_decay=decoupled, max_grad_norm=max_norm,
                              store_clipped_grads=store, **kw)
    else:
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(group_split(ps, grouped), foreach=False, **kw)
    out = dict(grad=[], norm=[], grad_in=[])
    for it, gs in enumerate(grads):
        for k, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if skip == (it, k) else g.clone().to(device=device, dtype=dtype)
        out["grad_in"].append([None if p.grad is None else p.grad.clone() for p in ps])
        if hip:
            opt.step()
            if max_norm is not None:
                out["norm"].append(opt.last_grad_norm.clone())
        else:
            if max_norm is not None:
                out["norm"].append(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).clone())
            opt.step()
        out["grad"].append([None if p.grad is None else p.grad.clone() for p in ps])
        if hook is not None:
            hook(it, ps)
    out["p"] = [p.detach().clone() for p in ps]
    for kind in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        out[kind] = [opt.state[p][kind].clone() for p in ps if p in opt.state and kind in opt.state[p]]
    out["step"] = [float(opt.state[p]["step"]) if p in opt.state else None for p in ps]
    out["opt"], out["params"] = opt, ps
    return out


def flat(r, kind):
    ts = r[kind]
    if kind == "grad":
        ts = [g for step in ts for g in step if g is not None]
    return torch.cat([t.detach().double().cpu().reshape(-1) for t in ts]) if ts else torch.zeros(0, dtype=torch.float64)


def pooled(r, r64, kind):
    x, x64 = flat(r, kind), flat(r64, kind)
    assert x.shape == x64.shape, kind
    if x64.numel() == 0:
        return None
    return float((x - x64).abs().max()) / float(x64.abs().max())


def assert_bound(name, hip, t32, t64, kinds=KINDS):
    lines = []
    for kind in kinds:
        e_hip, e_32 = pooled(hip, t64, kind), pooled(t32, t64, kind)
        if e_hip is None:
            continue
        lines.append(f"{name} {kind}: err_hip {e_hip:.3e} err_torch32 {e_32:.3e} ratio "
                     f"{e_hip / e_32 if e_32 else float('nan'):.2f}")
        print(lines[-1])
        assert e_hip <= (FACTOR * e_32 if e_32 > 0.0 else EPS23), lines[-1]
    return lines


def assert_norms(hip, t64):
    assert len(hip["norm"]) == len(t64["norm"]) > 0
    for it, (n, n64) in enumerate(zip(hip["norm"], t64["norm"])):
        assert n.dtype == torch.float32 and n.is_cuda and n.shape == ()
        rel = abs(float(n.double().cpu()) - float(n64)) / float(n64)
        print(f"step {it}: norm {float(n):.9g} float64 {float(n64):.17g} rel {rel:.3e}")
        assert rel <= EPS23, (it, rel)


_REF = {}


def reference(key, init, grads, **cfg):
    """torch on the CPU in float64 and float32, computed once per configuration."""
    if key not in _REF:
        _REF[key] = (run(init, grads, hip=False, dtype=torch.float64, **cfg), run(init, grads, hip=False, **cfg))
    return _REF[key]


VARIANTS = [dict(decoupled=d, amsgrad=a, wd=w, max_norm=m)
            for d, a, w, m in itertools.product((False, True), (False, True), (0.0, 0.01), (None, 1.0))]
GROUPED = [dict(decoupled=False, amsgrad=False, wd=0.01, max_norm=1.0, grouped=True),
           dict(decoupled=True, amsgrad=True, wd=0.01, max_norm=1.0, grouped=True)]


def _id(cfg):
    return "-".join(f"{k}={v}" for k, v in cfg.items())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", VARIANTS + GROUPED, ids=_id)
def test_every_variant_matches_float64(cfg, cuda):
    init, grads = inputs()
    t64, t32 = reference(_id(cfg), init, grads, **cfg)
    hip = run(init, grads, hip=True, device=cuda, **cfg)
    torch.cuda.synchronize()
    kinds = KINDS if cfg["max_norm"] is not None else KINDS[:-1]
    assert_bound(_id(cfg), hip, t32, t64, kinds)
    assert hip["step"] == t32["step"]
    if cfg["max_norm"] is None:
        assert hip["opt"].last_grad_norm is None
        for a, b in zip(hip["grad"], hip["grad_in"]):  # without clipping the gradients are only read
            assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_norm_and_inactive_clipping(cuda):
    init, grads = inputs()
    cfg = dict(decoupled=True, amsgrad=True, wd=0.01, max_norm=1.0)
    t64, _ = reference(_id(cfg), init, grads, **cfg)
    hip = run(init, grads, hip=True, device=cuda, **cfg)
    assert_norms(hip, t64)
    below = [it for it, n in enumerate(t64["norm"]) if float(n) < 1.0]
    assert below == [0, 3]  # the 0.1 steps do not clip, the others do
    for it in range(len(grads)):
        same = all(torch.equal(a, b) for a, b in zip(hip["grad"][it], hip["grad_in"][it]))
        assert same == (it in below), it  # coefficient exactly 1: bitwise untouched
    # the coefficient itself, after the last step (a clipping one): max_norm / (norm + 1e-6)
    norm, coef = (float(v) for v in hip["opt"]._norm_coef.cpu())
    assert coef == float(torch.tensor(1.0) / (torch.tensor(norm) + 1e-6)) and coef < 1.0


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(cuda):
    init, grads = inputs()
    cfg = dict(decoupled=False, amsgrad=True, wd=0.01, max_norm=1.0)
    a = run(init, grads, hip=True, device=cuda, **cfg)
    b = run(init, grads, hip=True, device=cuda, **cfg)
    for kind in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "norm"):
        assert len(a[kind]) == len(b[kind]) > 0
        assert all(torch.equal(x, y) for x, y in zip(a[kind], b[kind])), kind
    for x, y in zip(a["grad"], b["grad"]):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


@pytest.mark.gpu
def test_a_parameter_without_gradient_is_skipped(cuda):
    init, grads = inputs()
    cfg = dict(decoupled=True, amsgrad=True, wd=0.01, max_norm=1.0, skip=(1, 7))  # step 2 of 4, the largest tensor
    t64, t32 = reference("skip", init, grads[:4], **cfg)
    hip = run(init, grads[:4], hip=True, device=cuda, **cfg)
    assert hip["step"] == t32["step"] and hip["step"][7] == 3.0 and hip["step"][1] == 4.0
    assert hip["grad"][1][7] is None
    assert_bound("skip", hip, t32, t64)
    assert_norms(hip, t64)
    # a parameter that never gets a gradient has no state, as in torch
    cfg = dict(decoupled=False, amsgrad=False, wd=0.0, max_norm=None)
    never = [[g if k != 4 else None for k, g in enumerate(gs)] for gs in grads[:2]]
    ps = [torch.nn.Parameter(t.clone().to(cuda)) for t in init]
    opt = optim.FusedAdam(ps, lr=LR)
    for gs in never:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(cuda)
        opt.step()
    assert ps[4] not in opt.state and torch.equal(ps[4].cpu(), init[4]) and float(opt.state[ps[5]]["step"]) == 2.0


@pytest.mark.gpu
def test_more_tensors_than_one_launch_carries(cuda):
    init, grads = make_inputs([(7,)] * 300, 3, seed=5, base=0.03)  # norms near 0.14 / 1.4 / 14
    cfg = dict(decoupled=True, amsgrad=True, wd=0.01, max_norm=1.0)
    t64 = run(init, grads, hip=False, dtype=torch.float64, **cfg)
    t32 = run(init, grads, hip=False, **cfg)
    hip = run(init, grads, hip=True, device=cuda, **cfg)
    assert_bound("300 tensors", hip, t32, t64)
    assert_norms(hip, t64)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_nonfinite_gradients_propagate_as_in_torch(value, cuda):
    shapes = [(5,), (21, 21), (4097,)]
    init, grads = make_inputs(shapes, 2, seed=3, base=0.01)
    grads[1][1][3, 4] = value
    cfg = dict(decoupled=False, amsgrad=True, wd=0.0, max_norm=1.0)
    t32 = run(init, grads, hip=False, **cfg)
    hip = run(init, grads, hip=True, device=cuda, **cfg)
    for kind in KINDS:
        x, y = flat(hip, kind), flat(t32, kind)
        assert torch.equal(torch.isnan(x), torch.isnan(y)), kind
        assert not torch.isinf(x).any(), kind
    bad = torch.isnan(flat(hip, "p"))
    n = sum(t.numel() for t in init)
    if value != value:  # a NaN norm gives a NaN coefficient: everything is NaN
        assert int(bad.sum()) == n and torch.isnan(hip["norm"][1])
    else:  # inf: coefficient 0, inf * 0 = NaN in exactly that element, zero gradients elsewhere
        assert int(bad.sum()) == 1 and bool(torch.isnan(hip["p"][1][3, 4])) and torch.isinf(hip["norm"][1])
        g = flat(dict(grad=[hip["grad"][1]]), "grad")
        assert int(torch.isnan(g).sum()) == 1 and float(g[~torch.isnan(g)].abs().max()) == 0.0
        ok = ~bad  # the finite elements took a step with zero gradients, as torch's did
        assert float((flat(hip, "p")[ok] - flat(t32, "p")[ok]).abs().max()) <= 1e-6


class _Net(torch.nn.Module):
    def __init__(self, init):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in init])
        self.register_buffer("table", torch.arange(6, dtype=torch.float32))
        self.register_buffer("count", torch.zeros((), dtype=torch.int64))


def ema_schedule(step_read, update_every, update_after_step, initted, beta=0.995, power=2 / 3):
    """The documented behaviour restated: None (nothing), 'copy', or the lerp weight."""
    if step_read % update_every != 0:
        return None
    if step_read <= update_after_step or not initted:
        return "copy"
    e = max(step_read + 1 - update_after_step - 1, 0)
    decay = 0.0 if e == 0 else min(max(1 - (1 + e) ** (-power), 0.0), beta)
    return 1.0 - decay


@pytest.mark.gpu
def test_ema_follows_the_float64_track(cuda):
    shapes = [(1,), (5,), (21, 21), (4097,), (CHUNK + 1,)]
    steps, every, after = 25, 2, 6
    init, grads = make_inputs(shapes, steps, seed=11)
    cfg = dict(decoupled=False, amsgrad=False, wd=0.0, max_norm=1.0)

    def track(dtype):  # the torch parameter track and the schedule restated over it
        avg, state = [t.clone().to(dtype) for t in init], dict(initted=False)

        def hook(it, ps):
            w = ema_schedule(it, every, after, state["initted"])
            if w == "copy":
                state["initted"] = True
                for a, p in zip(avg, ps):
                    a.copy_(p.detach())
            elif w is not None:
                for a, p in zip(avg, ps):
                    a.lerp_(p.detach(), w)
        run(init, grads, hip=False, dtype=dtype, hook=hook, **cfg)
        return avg

    avg64, avg32 = track(torch.float64), track(torch.float32)
    net = _Net(init).to(cuda)
    ema = optim.EMA(net, update_every=every, update_after_step=after)
    opt = optim.FusedAdam(net.parameters(), lr=LR, betas=BETAS, eps=EPS, max_grad_norm=1.0)
    copies, weights = [], []
    for it, gs in enumerate(grads):
        for p, g in zip(net.w, gs):
            p.grad = g.to(cuda)
        opt.step()
        net.table += 1.0
        net.count += 1
        ema.update()
        kind = ema_schedule(it, every, after, it > 0)
        if kind == "copy":
            copies.append(it)
            assert all(torch.equal(a, p) for a, p in zip(ema.ema_model.w, net.w)), it  # bitwise the live parameters
        if kind is not None:
            weights.append(kind)
            assert torch.equal(ema.ema_model.table, net.table) and int(ema.ema_model.count) == it + 1  # buffers: copied
    assert copies == [0, 2, 4, 6] and len(weights) == 13 and int(ema.step) == steps and bool(ema.initted)
    assert all(not p.requires_grad for p in ema.ema_model.parameters())
    got = dict(ema=[p.detach() for p in ema.ema_model.w])
    assert_bound("ema", got, dict(ema=avg32), dict(ema=avg64), kinds=("ema",))
    # the state dict round-trips, and the copy goes on identically
    twin = optim.EMA(_Net(init).to(cuda), update_every=every, update_after_step=after)
    twin.load_state_dict(copy.deepcopy(ema.state_dict()))
    assert twin._step == steps and twin._initted and all(torch.equal(a, b) for a, b in zip(twin.ema_model.w, ema.ema_model.w))


@pytest.mark.gpu
def test_store_clipped_grads_off_leaves_the_gradients(cuda):
    init, grads = inputs()
    cfg = dict(decoupled=True, amsgrad=True, wd=0.01, max_norm=1.0)
    a = run(init, grads, hip=True, device=cuda, **cfg)
    b = run(init, grads, hip=True, device=cuda, store=False, **cfg)
    for x, y in zip(b["grad"], b["grad_in"]):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert any(not torch.equal(u, v) for x, y in zip(a["grad"], a["grad_in"]) for u, v in zip(x, y))
    for kind in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "norm"):
        assert all(torch.equal(x, y) for x, y in zip(a[kind], b[kind])), kind


@pytest.mark.gpu
def test_refusals_on_the_device(cuda):
    from skeletondiffusion_amd._lib import SkelDiffError

    def one(p, g=None):
        p = torch.nn.Parameter(p)
        p.grad = torch.ones_like(p) if g is None else g
        return optim.FusedAdam([p], lr=LR, max_grad_norm=1.0)

    for opt in (one(torch.zeros(4, dtype=torch.float64, device=cuda)), one(torch.zeros(4, dtype=torch.bfloat16, device=cuda)),
                one(torch.zeros(4, 6, device=cuda).t()), one(torch.zeros(4, device=cuda), torch.ones(8, device=cuda)[::2])):
        with pytest.raises(SkelDiffError, match="runs on the HIP engine only"):
            opt.step()
    mixed = [torch.nn.Parameter(torch.zeros(3, device=cuda)), torch.nn.Parameter(torch.zeros(3))]
    for p in mixed:
        p.grad = torch.ones_like(p)
    with pytest.raises(SkelDiffError, match="runs on the HIP engine only"):
        optim.FusedAdam(mixed, lr=LR).step()


@pytest.mark.gpu
def test_stage1_step_end_to_end(cuda):
    """Three training steps of the 1.06 M-parameter autoencoder on the device (autoencode + L1 + backward
    on the HIP GRU path), once with FusedAdam and once with clip_grad_norm_ + torch.optim.AdamW: every
    parameter within 1e-3 x max of the other run (the tolerance of tests/test_training.py)."""
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    _, _, _, types = skeleton("h36m16")

    def model():
        m = AutoEncoder(node_types=torch.from_numpy(types), num_nodes=16, encoder_hidden_size=96, decoder_hidden_size=96,
                        latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1, output_size=3,
                        recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU", if_consider_hip=False)
        synthetic.fill_module_(m, 4321)
        return m.to(cuda)

    past = (torch.from_numpy(synthetic.normal((3, 5, 16, 3), seed=51)) * 0.3).to(cuda)
    y = (torch.from_numpy(synthetic.normal((3, 4, 16, 3), seed=52)) * 0.3).to(cuda)
    kw = dict(lr=1e-3, weight_decay=0.01, amsgrad=True)
    prev = training.set_hip_training(True)
    try:
        before = dict(training.CALLS)
        results = []
        for fused in (True, False):
            m = model()
            assert sum(p.numel() for p in m.parameters()) == 1055902
            opt = optim.FusedAdam(m.parameters(), decoupled_weight_decay=True, max_grad_norm=1.0, **kw) if fused else \
                torch.optim.AdamW(m.parameters(), **kw)
            norms = []
            for _ in range(3):
                opt.zero_grad(set_to_none=True)
                out, _, _ = m.autoencode(y, past, 4)
                torch.nn.functional.l1_loss(out, y).backward()
                if fused:
                    opt.step()
                    norms.append(opt.last_grad_norm.clone())
                else:
                    norms.append(torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0))
                    opt.step()
            results.append(({n: p.detach().clone() for n, p in m.named_parameters()}, torch.stack(norms)))
        assert training.CALLS["gru_forward"] - before.get("gru_forward", 0) == 2 * 3 * 3
        assert training.CALLS["gru_backward"] - before.get("gru_backward", 0) == 2 * 3 * 2
    finally:
        training.set_hip_training(prev)
    (a, na), (b, nb) = results
    print("norms", na.tolist(), nb.tolist())
    assert torch.allclose(na, nb, rtol=1e-3, atol=0.0)
    moved = 0
    ref = model()
    for (n, p), q in zip(a.items(), ref.parameters()):
        assert float((p - b[n]).abs().max()) <= 1e-3 * float(b[n].abs().max()), n
        moved += int(not torch.equal(p, q.detach()))
    assert moved == len(a) == 23  # every tensor took the steps
