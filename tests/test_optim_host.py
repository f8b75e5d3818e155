"""Host side of the fused optimizer step: the C ABI and its argument checks, the
state-dict interchange with torch.optim.Adam / AdamW, the EMA schedule, the CPU refusals, and a
stand-alone program that walks the kernels' chunk arithmetic and compares their element math with a
restatement in double under AddressSanitizer.  No GPU; the device tests are in tests/test_gpu_optim.py."""
import copy
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import REPO
from skeletondiffusion_amd import _lib, optim
from skeletondiffusion_amd._lib import SkelDiffError

ENTRIES = ("sd_optim_workspace_bytes", "sd_optim_grad_norm", "sd_optim_adam_step", "sd_optim_ema_update")
CHUNK = 16384  # sd::optim::kChunk


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bsize_t sd_optim_workspace_bytes\(const int64_t\* numel, int32_t n_tensors\)", hdr)
    assert re.search(r"\bint sd_optim_grad_norm\(const float\* const\* grads, const int64_t\* numel, int32_t n_tensors", hdr)
    assert re.search(r"\bint sd_optim_adam_step\(const sd_optim_param\* params, int32_t n_tensors, double beta1", hdr)
    assert re.search(r"\bint sd_optim_ema_update\(float\* const\* ema, const float\* const\* params", hdr)
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    for lines in ("trainer.py:33", ":93-95", ":153", ":159", ":267-275"):  # the reference lines replaced
        assert lines in hdr, lines
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4
    # the binding's struct is the header's: nine 8-byte fields in the header's order
    fields = re.search(r"typedef struct sd_optim_param \{(.*?)\} sd_optim_param;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in _lib.SDOptimParam._fields_] and ctypes.sizeof(_lib.SDOptimParam) == 72
    for flag in ("AMSGRAD", "DECOUPLED_WD", "STORE_GRADS"):
        assert int(re.search(rf"#define SD_OPTIM_{flag} (\d+)", hdr).group(1)) == getattr(_lib, "SD_OPTIM_" + flag)


def test_host_argument_checks():
    """Every argument is refused by name on the host, before any device call."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 2)(p, p)
    null1 = (ctypes.c_void_p * 2)(p, None)
    numel = (ctypes.c_int64 * 2)(5, 3 * CHUNK + 3)
    neg = (ctypes.c_int64 * 2)(5, -1)
    assert L.sd_optim_workspace_bytes(numel, 2) == (1 + 4) * 8
    assert L.sd_optim_workspace_bytes(neg, 2) == 0 and L.sd_optim_workspace_bytes(None, 2) == 0

    def norm(grads=ptrs, numel=numel, n=2, max_norm=1.0, out=p, ws=p, ws_bytes=1 << 20):
        return L.sd_optim_grad_norm(grads, numel, n, max_norm, out, ws, ws_bytes, None)

    def params(**kw):
        arr = (_lib.SDOptimParam * 2)()
        for q in arr:
            q.p = q.grad = q.exp_avg = q.exp_avg_sq = q.max_exp_avg_sq = p
            q.numel, q.step, q.lr, q.weight_decay = 7, 1, 1e-3, 0.0
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return arr

    def step(arr=None, n=2, beta1=0.9, beta2=0.999, eps=1e-8, flags=_lib.SD_OPTIM_AMSGRAD, coef=None, **kw):
        return L.sd_optim_adam_step(params(**kw) if arr is None else arr, n, beta1, beta2, eps, flags, coef, None)

    def ema(a=ptrs, b=ptrs, numel=numel, n=2, w=0.5):
        return L.sd_optim_ema_update(a, b, numel, n, w, None)

    nan = float("nan")
    for call, cases in (
            (norm, ((dict(grads=None), b"grads is null"), (dict(grads=null1), b"grads[1] is null"),
                    (dict(numel=None), b"numel is null"), (dict(numel=neg), b"numel[1] < 0"), (dict(out=None), b"norm_coef is null"),
                    (dict(max_norm=0.0), b"max_norm"), (dict(max_norm=-1.0), b"max_norm"), (dict(max_norm=nan), b"max_norm"),
                    (dict(ws=None), b"workspace"), (dict(ws_bytes=5 * 8 - 1), b"workspace"), (dict(n=-1), b"n_tensors"))),
            (step, ((dict(arr=ctypes.c_void_p(None)), b"params is null"), (dict(p=None), b"params[1].p is null"),
                    (dict(grad=None), b"params[1].grad is null"), (dict(exp_avg=None), b"params[1].exp_avg is null"),
                    (dict(exp_avg_sq=None), b"params[1].exp_avg_sq is null"),
                    (dict(max_exp_avg_sq=None), b"params[1].max_exp_avg_sq is null"), (dict(numel=-3), b"params[1].numel < 0"),
                    (dict(lr=-1e-3), b"params[1].lr < 0"), (dict(lr=nan), b"params[1].lr < 0"),
                    (dict(weight_decay=-0.1), b"params[1].weight_decay < 0"), (dict(step=0), b"params[1].step < 1"),
                    (dict(beta1=1.0), b"beta1 outside"), (dict(beta1=-0.1), b"beta1 outside"), (dict(beta2=1.0), b"beta2 outside"),
                    (dict(beta2=nan), b"beta2 outside"), (dict(eps=-1e-8), b"eps < 0"), (dict(flags=8), b"flags"),
                    (dict(n=-1), b"n_tensors"))),
            (ema, ((dict(a=None), b"ema is null"), (dict(b=None), b"params is null"), (dict(a=null1), b"ema[1] is null"),
                   (dict(b=null1), b"params[1] is null"), (dict(numel=None), b"numel is null"), (dict(numel=neg), b"numel[1] < 0"),
                   (dict(w=-0.1), b"weight"), (dict(w=1.5), b"weight"), (dict(n=-1), b"n_tensors")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())
    # no tensors, and tensors of no elements, are a successful no-op (nothing is launched: the pointers
    # above are host addresses)
    zero = (ctypes.c_int64 * 2)(0, 0)
    nulls = (ctypes.c_void_p * 2)(None, None)
    assert norm(n=0, grads=None, numel=None, out=None, ws=None, ws_bytes=0) == 0
    assert step(n=0, arr=ctypes.c_void_p(None)) == 0
    assert ema(n=0, a=None, b=None, numel=None) == 0
    empty = (_lib.SDOptimParam * 2)()
    for q in empty:
        q.numel, q.step, q.lr = 0, 1, 1e-3
    assert L.sd_optim_adam_step(empty, 2, 0.9, 0.999, 1e-8, 0, None, None) == 0
    assert L.sd_optim_ema_update(nulls, nulls, zero, 2, 0.5, None) == 0


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((3,), (4, 5), (1,), (2, 2))]


def _three_steps(opt, ps, seed=1):
    """Three steps with gradients on all but the last parameter (which never gets one); the third
    step leaves ps[2] out as well, so that the step counts differ."""
    g = torch.Generator().manual_seed(seed)
    for it in range(3):
        for k, p in enumerate(ps[:-1]):
            p.grad = None if (it == 2 and k == 2) else torch.randn(p.shape, generator=g)
        opt.step()


def _assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert list(a["state"].keys()) == list(b["state"].keys())
    for k in a["state"]:
        assert list(a["state"][k].keys()) == list(b["state"][k].keys()), k
        for name, t in a["state"][k].items():
            u = b["state"][k][name]
            assert torch.is_tensor(u) and t.dtype == u.dtype and t.shape == u.shape and torch.equal(t, u), (k, name)


@pytest.mark.parametrize("cls,kw", [(torch.optim.AdamW, dict(amsgrad=True, weight_decay=0.01)),
                                    (torch.optim.Adam, dict(weight_decay=0.0))])
def test_state_interchange_with_torch(cls, kw):
    ps = _params()
    groups = [dict(params=ps[:2], lr=1e-3), dict(params=ps[2:], lr=5e-4, weight_decay=0.02)]
    ref = cls(groups, **kw)
    _three_steps(ref, ps)
    sd = copy.deepcopy(ref.state_dict())  # load_state_dict keeps the tensors it is given: no sharing with ref
    assert [float(sd["state"][k]["step"]) for k in sorted(sd["state"])] == [3.0, 3.0, 2.0] and 3 not in sd["state"]

    mine = optim.FusedAdam([dict(params=ps[:2]), dict(params=ps[2:])], lr=1.0)  # constructed on the CPU
    mine.load_state_dict(sd)
    assert mine.param_groups[1]["lr"] == 5e-4 and mine.param_groups[1]["weight_decay"] == 0.02
    assert mine.param_groups[0]["decoupled_weight_decay"] == (cls is torch.optim.AdamW)
    assert mine.param_groups[0]["amsgrad"] == kw.get("amsgrad", False)
    back = copy.deepcopy(mine.state_dict())
    _assert_same_state_dict(sd, back)

    fresh = cls([dict(params=ps[:2]), dict(params=ps[2:])], lr=1.0)
    fresh.load_state_dict(back)
    _assert_same_state_dict(sd, fresh.state_dict())
    # and the torch optimizer goes on from it exactly as the one that never left
    g = torch.Generator().manual_seed(9)
    grads = [torch.randn(p.shape, generator=g) for p in ps]
    before = [p.detach().clone() for p in ps]
    results = []
    for o in (ref, fresh):
        for p, b, gr in zip(ps, before, grads):
            p.data.copy_(b)
            p.grad = gr.clone()
        o.step()
        results.append([p.detach().clone() for p in ps])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_fresh_state_dict_has_torchs_layout():
    ps = _params()
    mine = optim.FusedAdam(ps, lr=1e-3, amsgrad=True, decoupled_weight_decay=True, weight_decay=0.01, max_grad_norm=1.0)
    ref = torch.optim.AdamW(ps, lr=1e-3, amsgrad=True, weight_decay=0.01)
    assert mine.state_dict()["param_groups"] == ref.state_dict()["param_groups"]
    assert mine.state_dict()["state"] == {}
    sched = torch.optim.lr_scheduler.StepLR(mine, step_size=1, gamma=0.5)  # an LR scheduler drives the groups
    mine.step()  # no gradients: nothing to do, on any device
    sched.step()
    assert mine.param_groups[0]["lr"] == 5e-4
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-1.0),
                dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            optim.FusedAdam(ps, **bad)


def test_cpu_parameters_are_refused_by_name():
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    opt = optim.FusedAdam(ps, lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(SkelDiffError, match="runs on the HIP engine only"):
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(ps, before)) and len(opt.state) == 0
    for p in ps:
        p.grad = None
    assert opt.step() is None  # nothing to do is no error anywhere
    model = torch.nn.Linear(3, 2)
    ema = optim.EMA(model, update_every=1)
    with pytest.raises(SkelDiffError, match="runs on the HIP engine only"):
        ema.update()
    assert int(ema.step) == 0 and not bool(ema.initted)


def test_ema_schedule_and_state_dict():
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    ema = optim.EMA(model, beta=0.995, update_every=10, update_after_step=100, power=2 / 3, inv_gamma=1.0)
    assert ema.ema_model is not model and all(not p.requires_grad for p in ema.ema_model.parameters())
    assert all(p.requires_grad for p in model.parameters())
    keys = list(ema.state_dict().keys())
    assert set(keys) == {"ema_model." + k for k in model.state_dict()} | {"initted", "step"}

    def decay_at(e, **kw):
        x = optim.EMA(model, **kw) if kw else ema
        x._step = x.update_after_step + 1 + e
        return x.get_current_decay()

    for s in (0, 1, 50, 100, 101):  # e = max(step - 101, 0) = 0
        ema._step = s
        assert ema.get_current_decay() == 0.0
    assert decay_at(1) == pytest.approx(1 - 2 ** (-2 / 3), rel=1e-15)
    assert decay_at(7) == pytest.approx(0.75, rel=1e-12)
    assert decay_at(26) == pytest.approx(8 / 9, rel=1e-12)
    e_cap = 2828  # (1 + e)^(2/3) >= 200 from e = 2828 on (2829^(2/3) = 200.03)
    assert decay_at(e_cap - 1) < 0.995 and decay_at(e_cap) == 0.995 and decay_at(10 ** 6) == 0.995
    assert decay_at(1, beta=0.995, min_value=0.5) == 0.5 and decay_at(7, beta=0.995, min_value=0.5) == pytest.approx(0.75)
    assert decay_at(0, beta=0.995, min_value=0.5) == 0.0
    assert decay_at(3, beta=0.995, power=1.0, inv_gamma=2.0) == pytest.approx(1 - 1 / 2.5)

    # update() acts only when the step it reads is a multiple of update_every
    acted = []
    x = optim.EMA(model, update_every=3, update_after_step=4)
    x._pairs = lambda: None
    x._blend = lambda pairs, w: acted.append((x._step - 1, w))
    for _ in range(13):
        x.update()
    assert [s for s, _ in acted] == [0, 3, 6, 9, 12] and int(x.step) == 13
    # step 0 and 3 are <= update_after_step: copies; 6 the first average (already initialised by the copies)
    assert [w for _, w in acted[:2]] == [1.0, 1.0]
    for s, w in acted[2:]:
        assert w == pytest.approx(1 - (1 - (1 + (s + 1 - 4 - 1)) ** (-2 / 3)) if s + 1 - 5 > 0 else 1.0)
    # the host counters follow a loaded state dict
    y = optim.EMA(model, update_every=3, update_after_step=4)
    y.load_state_dict(x.state_dict())
    assert y._step == 13 and y._initted is True and y.get_current_decay() == x.get_current_decay()


def test_chunk_walk_and_update_math_under_asan(tmp_path):
    """tests/host/optim_emulation.cpp walks the launch tables of tensors of 0, 1, 3, 5, 30, 441, one
    chunk - 1, one chunk, one chunk + 1 and three chunks + 3 elements (and more tensors than one
    launch carries) with the kernels' index arithmetic at 4-, 8- and 16-byte alignment, asserts that
    every element is visited once, and compares every variant's float32 update with a restatement in
    double; AddressSanitizer + UBSan, linked statically into a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "optim_emulation")
    src = os.path.join(REPO, "tests", "host", "optim_emulation.cpp")
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "optim emulation ok (48 variants)" in r.stdout
