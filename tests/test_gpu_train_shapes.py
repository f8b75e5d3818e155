"""The training kernels of csrc/sd_train.hip off the release Denoiser's shapes (tests/test_training.py runs
K, N in {96, 192, 384, 768}, dim_head in {32, 64}, C in {96, 192, 1024}).

Graph-linear, exact mode: integer-valued inputs (train_cases: every partial sum is exact in float32 while the
largest sum of |terms| stays below 2^22, asserted per case), so y, dx, dW, dbias and dghat must be
`torch.equal` to float64 autograd -- no tolerance.  The table (train_cases.GL_CASES, one branch per line) reaches
k_gemm<false>, ragged K tiles, the N = 3 clamp, every dW split count up to the 32-split cap with empty splits,
both forms of sum_parts, the scalar and 16-B forms of k_dghat_part<1> / <2> and k_dghat_part16, k_mix<4 / 8 / 16>
and the matrix-core mixing pass forward and transposed.  Variants: an unused weight type (exact zeros), one type
for all nodes, shared weights, no bias, every subset of wanted gradients, operands at a 4-byte storage offset.
Random mode: the same table with uniform inputs and a fully random G behind F.normalize, float64 autograd under
tests/test_training.py's own yardstick (REL_TOL, _close).
Then the attention core, FiLM + tanh, RMSNorm, the Mahalanobis loss and l1norm_rows at odd and minimal sizes
under that yardstick, guard bands round every output and the workspace through the C ABI, and one training step
of the J = 51 release Denoiser against the CPU torch path."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_training as TT
import train_cases as C
from conftest import build_release_diffusion, golden, release_inputs
from skeletondiffusion_amd import _lib, synthetic, training

pytestmark = pytest.mark.gpu

OUTPUTS = ("y", "dx", "dW", "dbias", "dghat")


# ---- graph-linear, exact mode ------------------------------------------------------------------------------------

def _off4(t, dev):
    """A contiguous float32 device copy of t whose storage starts 4 bytes into a 16-B aligned allocation."""
    buf = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


def _device_run(c, dev, need=("x", "W", "b", "gh"), offset=()):
    """training.graph_linear forward + backward on the exact case c.  `need`: the leaves that require grad;
    `offset`: which of x, W, dy sit at a 4-byte storage offset.  Returns the five outputs (None where absent)."""
    put = lambda name, t: (_off4(t, dev) if name in offset else t.float().to(dev))
    x, W, gh = put("x", c.x), put("W", c.W), put("gh", c.gh)
    b = None if c.b is None else put("b", c.b)
    for name, t in (("x", x), ("W", W), ("b", b), ("gh", gh)):
        if t is not None and name in need:
            t.requires_grad_(True)
    y = training.graph_linear(x, W, b, gh, None if c.types is None else c.types.to(dev))
    dy = put("dy", c.dy)
    seen = []
    y.register_hook(lambda g: seen.append(g.data_ptr()))
    y.backward(dy)
    torch.cuda.synchronize()
    assert seen == [dy.data_ptr()]  # the backward got this very tensor (its alignment with it)
    return dict(y=y.detach(), dx=x.grad, dW=W.grad, dbias=None if b is None else b.grad, dghat=gh.grad)


def _assert_exact_condition(c):
    assert c.sum_abs < C.LIMIT, f"sum of |terms| {c.sum_abs:.4g} >= 2^22: float32 may round, the case proves nothing"
    if c.gh.shape[0] >= 2:
        assert (c.gh < 0).any() and not torch.equal(c.gh, c.gh.t())
        assert torch.equal(c.gh * 2, (c.gh * 2).round()) and float(c.gh.abs().max()) <= 1.0


def _assert_equals_reference(got, c):
    for k in OUTPUTS:
        ref = c.ref[k]
        if ref is None:
            assert got[k] is None, k
            continue
        g = got[k].double().cpu()
        assert g.shape == ref.shape, k
        assert torch.equal(g, ref), (f"{k}: {int((g != ref).sum())} of {ref.numel()} elements differ, "
                                     f"max |diff| {float((g - ref).abs().max())}, first at "
                                     f"{tuple(int(v) for v in (g != ref).nonzero()[0])}")


@pytest.mark.parametrize("case", C.GL_CASES, ids=C.case_id)
def test_gl_exact(case, cuda):
    c = C.exact_case(case)
    _assert_exact_condition(c)
    _assert_equals_reference(_device_run(c, cuda), c)


@pytest.mark.parametrize("case,variant", C.VARIANT_CASES, ids=[C.case_id(c) + "-" + C.variant_id(v) for c, v in C.VARIANT_CASES])
def test_gl_exact_variants(case, variant, cuda):
    """An unused type's dW[t] and dbias[t] are exactly zero (k_gemm's type mode finds no node, k_dbias_part adds
    nothing); one type for all nodes; shared weights; no bias."""
    c = C.exact_case(case, variant)
    _assert_exact_condition(c)
    got = _device_run(c, cuda)
    _assert_equals_reference(got, c)
    unused = [t for t in range(max(1, c.n_types)) if t not in c.used]
    assert bool(unused) == (variant.extra_type or variant.one_type)
    for t in unused:
        assert float(c.ref["dW"][t].abs().max()) == 0.0 and float(got["dW"][t].abs().max()) == 0.0, t
        if c.b is not None:
            assert float(c.ref["dbias"][t].abs().max()) == 0.0 and float(got["dbias"][t].abs().max()) == 0.0, t


SUBSETS = [("x",), ("gh",), ("W", "b"), ("W", "b", "gh")]  # only x; only ghat; only W and bias; x without grad


@pytest.mark.parametrize("case", C.SUBSET_CASES, ids=C.case_id)
def test_gl_exact_gradient_subsets(case, cuda):
    """A backward with only some outputs wanted (sd_gl_train_backward's null dx / dW / dbias / dghat and its
    early return): the gradients present equal the full call's bit for bit, the others are None."""
    c = C.exact_case(case)
    _assert_exact_condition(c)
    full = _device_run(c, cuda)
    _assert_equals_reference(full, c)
    leaf_of = dict(dx="x", dW="W", dbias="b", dghat="gh")
    for need in SUBSETS:
        got = _device_run(c, cuda, need=need)
        assert torch.equal(got["y"], full["y"]), need
        for k, leaf in leaf_of.items():
            if leaf in need:
                assert torch.equal(got[k], full[k]), (need, k)
            else:
                assert got[k] is None, (need, k)


@pytest.mark.parametrize("case", C.OFFSET_CASES, ids=C.case_id)
def test_gl_exact_unaligned_operands(case, cuda):
    """x, W and dy as contiguous views 4 bytes into their storage (`.contiguous()` keeps such a view, the ABI
    states no alignment): every 16-B path must decline (gemm_vec_ok, launch_mix_mfma, the dghat dispatch's
    alignment predicate) and the results equal the aligned call's bit for bit."""
    c = C.exact_case(case)
    _assert_exact_condition(c)
    full = _device_run(c, cuda)
    _assert_equals_reference(full, c)
    for offset in (("x",), ("W",), ("dy",), ("x", "W", "dy")):
        got = _device_run(c, cuda, offset=offset)
        for k in OUTPUTS:
            assert torch.equal(got[k], full[k]), (offset, k)


# ---- graph-linear, random mode -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.RANDOM_CASES, ids=C.case_id)
def test_gl_random_vs_autograd(case, cuda):
    """At J = 1 G-hat = sign(G) and dG is identically zero: its two terms dghat / |G| and
    sign(G) dghat G / G^2 cancel, and a bound scaled by max |reference| = 0 would ask torch's float32
    F.normalize backward to cancel them without rounding (on the CPU it leaves 6e-8).  There dG is held to
    REL_TOL x the size of those terms; dghat, what the kernel writes, is compared in every case."""
    c = C.random_case(case)
    x, W, G, b = (t.float().to(cuda).requires_grad_(True) for t in (c.x, c.W, c.G, c.b))
    gh = F.normalize(G, p=1.0, dim=1)
    gh.retain_grad()
    y = training.graph_linear(x, W, b, gh, None if c.types is None else c.types.to(cuda))
    y.backward(c.dy.float().to(cuda))
    torch.cuda.synchronize()
    TT._close(y, c.ref["y"], "y")
    TT._close(x.grad, c.ref["dx"], "dx")
    TT._close(W.grad, c.ref["dW"], "dW")
    TT._close(gh.grad, c.ref["dghat"], "dghat")
    TT._close(b.grad, c.ref["dbias"], "dbias")
    if case[0] == 1:
        assert float(c.ref["dG"].abs().max()) == 0.0
        term = float((c.ref["dghat"] / c.G).abs().max())
        err = float(G.grad.abs().max())
        assert err <= TT.REL_TOL * term, f"dG: {err:.3e} vs cancelling terms of {term:.3e}"
    else:
        TT._close(G.grad, c.ref["dG"], "dG")


# ---- the other kernels, float64 autograd, the same yardstick -------------------------------------------------------

def _attention(qkv, dout, heads, dh, cuda):
    scale = dh ** -0.5
    ref_in = qkv.clone().requires_grad_(True)
    ref = TT._ref_attention(ref_in, heads, dh, scale)
    (ref * dout).sum().backward()
    x = qkv.float().to(cuda).requires_grad_(True)
    out = training.attention_core(x, heads, dh, scale)
    out.backward(dout.float().to(cuda))
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    TT._close(out, ref, "out")
    TT._close(x.grad, ref_in.grad, "dqkv")


def _attention_inputs(J, heads, dh, rows, seed=0):
    g = torch.Generator().manual_seed(J * 100 + heads * 10 + dh + rows + seed)
    return (torch.randn(rows, J, 3 * heads * dh, generator=g, dtype=torch.float64),
            torch.randn(rows, J, heads * dh, generator=g, dtype=torch.float64))


# odd dim_head; J J > 256 in the J x J loops (33, 64); one of everything; the release heads at an odd J
@pytest.mark.parametrize("J,heads,dh,rows", [(1, 1, 1, 1), (2, 3, 5, 3), (33, 1, 33, 2), (64, 2, 63, 1), (17, 8, 32, 1)])
def test_attention_core_shapes(J, heads, dh, rows, cuda):
    _attention(*_attention_inputs(J, heads, dh, rows), heads, dh, cuda)


def test_attention_core_large_logits(cuda):
    """qkv scaled by 30: the logits reach thousands, so exp overflows unless the row maximum is subtracted.  The
    inputs are conditioned so that the comparison stays sound in float32: in every softmax row the two largest
    logits lie more than 50 apart (asserted in float64), P is one-hot to e^-50 in either precision."""
    J, heads, dh, rows = 5, 2, 8, 2
    qkv, dout = _attention_inputs(J, heads, dh, rows, seed=3)
    qkv = qkv * 30
    q, k, _ = (c.reshape(rows, J, heads, dh) for c in qkv.chunk(3, dim=-1))
    logits = torch.einsum("bnhc,bjhc->bhnj", q * dh ** -0.5, k)
    top = logits.topk(2, dim=-1).values
    assert float(logits.max()) > 100.0  # past expf's overflow at 88.7
    assert float((top[..., 0] - top[..., 1]).min()) > 50.0
    _attention(qkv, dout, heads, dh, cuda)


def test_attention_core_equal_logits(cuda):
    """One query row of zeros: its logits are all equal, its softmax row uniform."""
    J, heads, dh, rows = 7, 2, 5, 2
    qkv, dout = _attention_inputs(J, heads, dh, rows, seed=4)
    qkv[1, 3, :heads * dh] = 0.0
    _attention(qkv, dout, heads, dh, cuda)


# C > 256: k_film_tanh_bwd's second, ragged column block (257, 300); one of everything
@pytest.mark.parametrize("rows,J,C_", [(3, 1, 1), (2, 64, 257), (1, 5, 300)])
def test_film_tanh_shapes(rows, J, C_, cuda):
    TT.test_film_tanh_vs_autograd(rows, J, C_)


# each with one all-zero vector (TT: x[0, J - 1]); C not a multiple of 64; (16, 16, 8): 16 workgroups, dg through
# k_sum_parts_wave; (15, 16, 8): 15 workgroups, the loop form
@pytest.mark.parametrize("rows,J,C_", [(1, 1, 1), (1, 17, 63), (3, 7, 65), (2, 5, 1000), (16, 16, 8), (15, 16, 8)])
def test_rmsnorm_shapes(rows, J, C_, cuda):
    TT.test_rmsnorm_vs_autograd(rows, J, C_)


# (2, 64, 255): the largest LDS carve with an odd F; (5, 3, 7): J F < 256, idle threads in the reduction
@pytest.mark.parametrize("mse", [False, True])
@pytest.mark.parametrize("pred_noise", [False, True])
@pytest.mark.parametrize("rows,J,F_", [(3, 1, 1), (2, 64, 255), (5, 3, 7)])
def test_mahalanobis_loss_shapes(rows, J, F_, pred_noise, mse, cuda):
    TT.test_mahalanobis_loss_vs_autograd(rows, J, F_, pred_noise, mse)


@pytest.mark.parametrize("J", [2, 63])
def test_l1norm_rows_negative_row(J, cuda):
    """F.normalize(G, p=1, dim=1) with one row of negative entries only (its norm is the negated sum)."""
    g = torch.Generator().manual_seed(J + 500)
    G = torch.randn(J, J, generator=g, dtype=torch.float64)
    G[J - 1] = -G[J - 1].abs() - 0.1
    dout = torch.randn(J, J, generator=g, dtype=torch.float64)
    Gr = G.clone().requires_grad_(True)
    ref = F.normalize(Gr, p=1.0, dim=1)
    (ref * dout).sum().backward()
    Gg = G.float().to(cuda).requires_grad_(True)
    out = training.l1norm_rows(Gg)
    out.backward(dout.float().to(cuda))
    torch.cuda.synchronize()
    TT._close(out, ref, "ghat")
    TT._close(Gg.grad, Gr.grad, "dG")


# ---- guard bands through the C ABI -------------------------------------------------------------------------------

PAD_BYTES = 4096 * 4  # a multiple of 16 B: the vector paths stay selected
SENTINEL = 0xA5


def _guarded(nfloats, dev):
    """(whole sentinel-filled byte buffer, its middle as `nfloats` float32, NaN-prefilled)."""
    whole = torch.full((2 * PAD_BYTES + 4 * nfloats,), SENTINEL, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 256 == 0
    mid = whole[PAD_BYTES:PAD_BYTES + 4 * nfloats].view(torch.float32)
    mid.fill_(float("nan"))
    return whole, mid


def _pads_intact(whole):
    return bool((whole[:PAD_BYTES] == SENTINEL).all()) and bool((whole[-PAD_BYTES:] == SENTINEL).all())


@pytest.mark.parametrize("case", C.GUARD_CASES, ids=C.case_id)
def test_gl_guard_bands(case, cuda):
    """sd_gl_train_forward / _backward with z, y, dx, dW, dbias and dghat each in the middle of a sentinel buffer,
    NaN-prefilled, and a NaN-prefilled workspace of exactly sd_gl_train_workspace_bytes inside another: no band
    changes, every output element is written (no NaN, so no unwritten partial was read either), and the
    exact-mode results equal the reference bit for bit."""
    J, K, N, nt, rows = case
    c = C.exact_case(case)
    _assert_exact_condition(c)
    L_ = _lib.lib()
    stream = torch.cuda.current_stream(cuda).cuda_stream
    x, W, b, gh, dy = (t.float().to(cuda).contiguous() for t in (c.x, c.W, c.b, c.gh, c.dy))
    types = c.types.to(cuda)
    nbytes = int(L_.sd_gl_train_workspace_bytes(rows, J, K, N, nt))
    assert nbytes == C.workspace_bytes(rows, J, K, N, nt)
    sizes = dict(z=rows * J * N, y=rows * J * N, dx=rows * J * K, dW=nt * N * K, dbias=nt * N, dghat=J * J, ws=nbytes // 4)
    whole, mid = {}, {}
    for k, n in sizes.items():
        whole[k], mid[k] = _guarded(n, cuda)
    _lib.check(L_.sd_gl_train_forward(x.data_ptr(), W.data_ptr(), b.data_ptr(), types.data_ptr(), nt, gh.data_ptr(), rows,
                                      J, K, N, mid["z"].data_ptr(), mid["y"].data_ptr(), stream))
    _lib.check(L_.sd_gl_train_backward(x.data_ptr(), mid["z"].data_ptr(), dy.data_ptr(), W.data_ptr(), types.data_ptr(),
                                       nt, gh.data_ptr(), rows, J, K, N, mid["dx"].data_ptr(), mid["dW"].data_ptr(),
                                       mid["dbias"].data_ptr(), mid["dghat"].data_ptr(), mid["ws"].data_ptr(), nbytes,
                                       stream))
    torch.cuda.synchronize()
    for k in sizes:
        assert _pads_intact(whole[k]), f"write outside {k}"
    for k in ("z",) + OUTPUTS:
        got = mid[k].double().cpu().reshape(c.ref[k].shape)
        assert not torch.isnan(got).any(), f"{k}: {int(torch.isnan(got).sum())} elements unwritten or from unwritten partials"
        assert torch.equal(got, c.ref[k]), k


# ---- a J = 51 training step --------------------------------------------------------------------------------------

def test_mano51_training_step_on_hip(cuda):
    """test_release_training_step_on_hip's comparison for the J = 51 release Denoiser (two rows): N = 192 and 768
    with J > 32 put both matrix-core mixing passes, dz = G-hat^T dy among them, on a real module path.  The fixture
    holds no train_loss: the loss is compared with the CPU torch path's, every parameter gradient likewise."""
    z = golden("release_mano51_T10")
    xcs, fu, start, _ = release_inputs(z)
    xc = xcs.repeat_interleave(fu, 0)
    B, J = start.shape[0], start.shape[1]
    assert J == 51
    t_train = torch.arange(B) % int(z["T"])
    noise = torch.from_numpy(synthetic.normal((B, J, 96), 24))
    xs = torch.from_numpy(synthetic.uniform((B, J, 96), 25))

    d_cpu = build_release_diffusion(z)
    loss_c, _, _ = d_cpu.p_losses(xs, t_train, noise=noise, x_cond=xc)
    loss_c.mean().backward()

    d_gpu = build_release_diffusion(z, device=cuda)
    assert training.hip_training_enabled()
    loss_g, _, _ = d_gpu.p_losses(xs.to(cuda), t_train.to(cuda), noise=noise.to(cuda), x_cond=xc.to(cuda))
    names = TT._grad_fn_names(loss_g)
    for fn in ("GraphLinearFunctionBackward", "AttentionCoreFunctionBackward", "FilmTanhFunctionBackward",
               "RMSNormFunctionBackward", "MahalanobisLossFunctionBackward", "L1NormRowsFunctionBackward"):
        assert fn in names, f"{fn}: HIP kernel not on the training path"
    loss_g.mean().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss_g.detach().cpu().numpy(), loss_c.detach().numpy(), atol=1e-5, rtol=1e-5)
    pc = dict(d_cpu.named_parameters())
    n_checked = 0
    for k, p in d_gpu.named_parameters():
        if pc[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        got, ref = p.grad.double().cpu(), pc[k].grad.double()
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-3 * scale + 1e-9, f"{k}: max |diff| {err:.3e} vs max |ref| {scale:.3e}"
        n_checked += 1
    assert n_checked > 100
