"""The selected-row best-of-k training step without a GPU: the two passes of
best_of_k.pick_best_loss_selected on torch ops in float64 against today's step (one forward +
backward over all b k rows, the trainer's min / gather selection), its refusals, the C ABI of
sd_q_sample_groups (header, binding, library, every host argument check) and the stand-alone host
emulation of the kernel's address arithmetic under AddressSanitizer + UBSan."""
import contextlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import oracle as O
from conftest import REPO, build_release_diffusion, golden
from skeletondiffusion_amd import _lib
from skeletondiffusion_amd.core import best_of_k as B

# relative L2 between the two steps' gradients: far above float64 reduction-order noise (2e-15 measured),
# far below any wrong row
GRAD_RTOL = 1e-9


def full_step_reference(d, data, x_cond, k, t, noise):
    """pick_best_loss's body (latent_space) at a fixed t and noise: p_losses over all b k rows under
    autograd, then the trainer's selection (trainer.py:218-220, oracle.best_of_k: min + gather) and
    (loss * loss_weight).mean()."""
    loss, w, _ = d.p_losses(data, t, noise=noise, x_cond=x_cond, n_train_samples=k)
    sel, idx = O.best_of_k(loss, k)
    return (sel * w).mean(), idx


def grads_of(d, loss):
    for p in d.parameters():
        p.grad = None
    loss.backward()
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in d.named_parameters()}


def assert_same_step(d, data, x_cond, k, t, noise, n_params):
    ref_loss, ref_idx = full_step_reference(d, data, x_cond, k, t, noise)
    g_ref = grads_of(d, ref_loss)
    loss, idx = B.pick_best_loss_selected(d, data, x_cond, k, similarity_space="latent_space", t=t, noise=noise)
    g_sel = grads_of(d, loss)
    np.testing.assert_array_equal(idx.numpy(), ref_idx.numpy())
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-14 * max(1.0, abs(float(ref_loss.detach())))
    assert len(g_ref) == n_params
    worst = 0.0
    for name, g in g_ref.items():
        assert g is not None and g_sel[name] is not None, name
        assert float(g.norm()) > 0, name
        rel = float((g_sel[name] - g).norm() / g.norm())
        worst = max(worst, rel)
        assert rel <= GRAD_RTOL, (name, rel)
    return worst


@contextlib.contextmanager
def float64_default():
    """float64 as torch's default dtype while a .double() model runs (it is built in float32 first):
    the Denoiser's sinusoidal time embedding is formed in the default dtype."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def fixture_inputs(dtype=torch.float64):
    z = golden("best_of_k")
    data, x_cond, noise = (torch.from_numpy(z[n]).to(dtype) for n in ("data", "x_cond", "noise"))
    return z, data, x_cond, torch.from_numpy(z["t"]), noise, int(z["k"])


def test_selected_step_gradients_equal_full_step():
    """The release Denoiser in float64 on tests/golden/best_of_k.npz (b = 3, k = 4): the scalar, the
    indices and all 119 parameter gradients of the selected-row step equal the full step's."""
    z, data, x_cond, t, noise, k = fixture_inputs()
    d = build_release_diffusion(golden("release_h36m16_T10")).double().train()
    with float64_default():
        assert_same_step(d, data, x_cond, k, t, noise, n_params=119)
        loss, idx = B.pick_best_loss_selected(d, data, x_cond, k, t=t, noise=noise)
    np.testing.assert_array_equal(idx.numpy(), z["idx_latent"])


def test_selected_step_isotropic_pred_noise():
    """IsotropicGaussianDiffusion(pred_noise) over the README Denoiser: the target of the selected pass
    is the noise of the chosen copy."""
    from skeletondiffusion_amd import synthetic
    from skeletondiffusion_amd.core.diffusion import IsotropicGaussianDiffusion
    from skeletondiffusion_amd.core.network import Denoiser

    _, data, _, t, noise, k = fixture_inputs()
    m = Denoiser(dim=96, cond_dim=0, out_dim=96, channels=16, num_nodes=16)
    synthetic.fill_module_(m, 1234)
    d = IsotropicGaussianDiffusion(model=m, diffusion_timesteps=10, diffusion_objective="pred_noise").double().train()
    assert d.objective == "pred_noise"
    with float64_default():
        assert_same_step(d, data, None, k, t, noise, n_params=len(list(d.parameters())))


def test_selected_step_k1_and_default_noise():
    """k = 1 runs the selected pass only (no index, as pick_best_loss); without t / noise the step
    draws them and still returns a finite scalar with a gradient."""
    _, data, x_cond, t, noise, k = fixture_inputs()
    d = build_release_diffusion(golden("release_h36m16_T10")).double().train()
    with float64_default():
        loss, idx = B.pick_best_loss_selected(d, data, x_cond, 1, t=t, noise=noise[::k].contiguous())
        ref, w, _ = d.p_losses(data, t, noise=noise[::k].contiguous(), x_cond=x_cond, n_train_samples=1)
        assert idx is None and abs(float(loss.detach()) - float((ref * w).mean().detach())) < 1e-14
        torch.manual_seed(5)
        loss, idx = B.pick_best_loss_selected(d, data, x_cond, 3)
    assert idx.shape == (3,) and int(idx.min()) >= 0 and int(idx.max()) < 3
    assert torch.isfinite(loss) and loss.grad_fn is not None


def test_selected_step_refusals_name_the_cause():
    from skeletondiffusion_amd.core.diffusion import NonisotropicGaussianDiffusion
    from skeletondiffusion_amd.core.network import Denoiser
    from conftest import pinned_cov

    _, data, x_cond, t, noise, k = fixture_inputs(torch.float32)
    d = build_release_diffusion(golden("release_h36m16_T10")).train()
    with pytest.raises(ValueError, match="noise"):
        B.pick_best_loss_selected(d, data, x_cond, k, t=t, noise=noise[:-1])
    with pytest.raises(ValueError, match="noise"):
        B.pick_best_loss_selected(d, data, x_cond, k + 1, t=t, noise=noise)
    d.model.layers[0][1].fn.fn.attn_dropout.p = 0.1
    with pytest.raises(ValueError, match="Dropout.*attn_dropout"):
        B.pick_best_loss_selected(d, data, x_cond, k, t=t, noise=noise)
    d.eval()  # the dropout is inactive in eval mode
    B.pick_best_loss_selected(d, data, x_cond, k, t=t, noise=noise)
    S, L, U = pinned_cov(16)
    m = Denoiser(dim=96, cond_dim=0, out_dim=96, channels=16, num_nodes=16, self_condition=True)
    sc = NonisotropicGaussianDiffusion(Sigma_N=S, Lambda_N=L, U=U, model=m, timesteps=10)
    with pytest.raises(ValueError, match="self_condition"):
        B.pick_best_loss_selected(sc, data, None, k, t=t, noise=noise)
    with pytest.raises(AssertionError, match="Similarity space"):
        B.pick_best_loss_selected(d, data, x_cond, k, similarity_space="pixel_space", t=t, noise=noise)


def test_selected_step_keeps_a_models_own_white_noise():
    """A diffusion that overrides get_white_noise is fed its own noise, as under p_losses, once for all
    b k rows and the same in both passes: the step equals the one given that noise as a tensor."""
    _, data, x_cond, t, noise, k = fixture_inputs()
    d = build_release_diffusion(golden("release_h36m16_T10")).double().train()
    calls = []

    class OwnNoise(type(d)):
        def get_white_noise(self, x, *args, **kwargs):
            calls.append(tuple(x.shape))
            return 0.5 * noise

    d.__class__ = OwnNoise
    with float64_default():
        loss, idx = B.pick_best_loss_selected(d, data, x_cond, k)  # t drawn, noise the model's own
        loss, idx = B.pick_best_loss_selected(d, data, x_cond, k, t=t)
        want, want_idx = B.pick_best_loss_selected(d, data, x_cond, k, t=t, noise=0.5 * noise)
    assert calls == [tuple(noise.shape)] * 2
    assert torch.equal(idx, want_idx) and torch.equal(loss.detach(), want.detach())


def test_forward_only_flag_is_thread_local_and_off_by_default():
    import threading

    from skeletondiffusion_amd import training

    assert not training.hip_forward_only_active()
    with torch.no_grad():
        assert not training.hip_gate()
        with training.hip_forward_only():
            assert training.hip_forward_only_active() and training.hip_gate()
            seen = []
            th = threading.Thread(target=lambda: seen.append(training.hip_forward_only_active()))
            th.start()
            th.join()
            assert seen == [False]
            with training.hip_forward_only():
                pass
            assert training.hip_forward_only_active()  # the inner exit restores the outer state
        assert not training.hip_gate()
    assert training.hip_gate() and not training.hip_forward_only_active()


# ---- sd_q_sample_groups: header, binding, library, host argument checks ---------------------------

def test_q_sample_entry_is_declared_bound_and_exported():
    from test_abi import declared_symbols

    assert "sd_q_sample_groups" in declared_symbols()
    assert "sd_q_sample_groups" in _lib.EXPORTED
    lib = _lib.lib()
    assert hasattr(lib, "sd_q_sample_groups")
    assert lib.sd_abi_version() == 4  # additive: the ABI number stays


def _call(**over):
    """sd_q_sample_groups with valid host-side arguments (fake non-null, aligned pointers: every
    refusal below happens before any device call), overridden by name."""
    a = dict(x0=0x1000, t=0x2000, sqrt_ac=0x3000, M=0x4000, sqrt_1mac=None, T=10, nseq=3, k=4, J=16, D=96, sel=None,
             noise_in=None, seed=7, step=0, row0=0, x_t=0x5000, noise_out=None)
    a.update(over)
    lib = _lib.lib()
    rc = lib.sd_q_sample_groups(a["x0"], a["t"], a["sqrt_ac"], a["M"], a["sqrt_1mac"], a["T"], a["nseq"], a["k"], a["J"],
                                a["D"], a["sel"], a["noise_in"], a["seed"], a["step"], a["row0"], a["x_t"],
                                a["noise_out"], None)
    return rc, lib.sd_last_error() or b""


@pytest.mark.parametrize("over, name", [
    (dict(x0=None), b"x0"), (dict(t=None), b"t is null"), (dict(sqrt_ac=None), b"sqrt_alphas_cumprod"),
    (dict(x_t=None), b"x_t"), (dict(k=0), b"k must"), (dict(J=0), b"J must"), (dict(J=65), b"J must"),
    (dict(D=0), b"D must"), (dict(D=98), b"D must"), (dict(D=260), b"D must"), (dict(T=0), b"T must"),
    (dict(step=-1), b"step"), (dict(step=2 ** 31), b"step"), (dict(row0=-1), b"row0"), (dict(nseq=-1), b"nseq"),
    (dict(M=None), b"exactly one of M and sqrt_one_minus_alphas_cumprod"),
    (dict(sqrt_1mac=0x6000), b"exactly one of M and sqrt_one_minus_alphas_cumprod"),
    (dict(x0=0x1004), b"x0 must be 16-byte aligned"), (dict(x_t=0x5008), b"x_t must be 16-byte aligned"),
    (dict(noise_in=0x7004), b"noise_in"), (dict(noise_out=0x8004), b"noise_out"),
    (dict(nseq=2 ** 30, k=4), b"nseq times k"),
])
def test_q_sample_host_checks_name_the_argument(over, name):
    rc, msg = _call(**over)
    assert rc == -1 and b"q_sample_groups" in msg and name in msg, (rc, msg)


def test_q_sample_no_sequences_is_a_no_op():
    assert _call(nseq=0, x0=None, t=None, x_t=None)[0] == 0
    assert _call(nseq=0, M=None, sqrt_1mac=0x6000)[0] == 0


def test_q_sample_binding_refuses_host_tensors():
    from skeletondiffusion_amd import training

    x0 = torch.zeros(2, 16, 96)
    with pytest.raises(ValueError, match="x0"):
        training.q_sample_groups(x0, torch.zeros(2, dtype=torch.long), torch.ones(10), 4, M=torch.zeros(10, 16, 16))


# ---- the kernel's address arithmetic on the host ---------------------------------------------------

def test_q_sample_addresses_and_arithmetic_under_asan(tmp_path):
    """tests/host/q_sample_emulation.cpp walks sd_q_sample_addr.h over (nseq, k, J, D) in (1,1,1,4),
    (3,4,16,96), (2,50,17,96), (5,7,21,96), (1,3,51,96), (2,2,64,256), both forms, with and without
    sel and with supplied noise: every output element written once, every (row, quad) on the full
    launch's Philox counter, the sums equal to a restatement in double; AddressSanitizer + UBSan,
    linked statically into a program of its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "q_sample_emulation")
    src = os.path.join(REPO, "tests", "host", "q_sample_emulation.cpp")
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "q_sample emulation ok (48 launches" in r.stdout
