"""The split route's GEMM phases store Y straight from swapped-operand MFMA accumulators
(DESIGN.md §4x): k_gl4t (route 3) and k_gl4y (route 2) run every 32x32x16 MFMA with the weight
fragment as A and the x fragment as B, so a lane holds one batch row and 16-B pieces of columns, and
the tile goes to memory in 4 dwordx4 stores with no LDS transpose.  Per output element the products
and their order are unchanged, so both routes must still equal the one-kernel route (route 1, which
this change does not touch) bit for bit.

Rows: 33 (the second 32-row tile has one live row; an RT = 2 wave holds a live and a dead tile;
three waves of the workgroup are dead) and 257 (a second row group with one live row).
Bias: bias[type, col] = (1000 type + col) / 4096 -- every (type, column) its own value, so a bias
permuted between columns or shifted between the two lane halves cannot cancel.
The layer hook carries no status word; the status flag of the range fallback is asserted on the
engine-level cases."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O
from skeletondiffusion_amd import _lib

pytestmark = pytest.mark.gpu

ROWS = (33, 257)
# (J, node types, K1, K2, N, rms)
SHAPES = [
    (16, 10, 192, 0, 96, False),
    (16, 10, 192, 0, 192, False),
    (16, 10, 256, 0, 192, False),
    (16, 10, 192, 192, 192, False),  # the x1 -> x2 switch
    (16, 10, 192, 0, 768, True),     # the per-lane RMS scale at CT = 6
    (17, 9, 192, 0, 192, False),
    (21, 13, 192, 0, 192, False),
]


@pytest.fixture
def split_route():
    L = _lib.lib()

    def set_(route):
        assert L.sd_test_set_split_route(route) >= 0

    yield set_
    L.sd_test_set_split_route(0)


def _inputs(J, nty, K1, K2, N, B):
    g = torch.Generator().manual_seed(J * 1000 + N + K1 + 7 * K2 + B)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    x1 = r(B, J, K1)
    x2 = r(B, J, K2) if K2 else None
    W = r(nty, N, K1 + K2) / (K1 + K2) ** 0.5
    types = torch.arange(J) % nty  # at least three node types, every type used
    bias = (1000.0 * torch.arange(nty)[:, None] + torch.arange(N)[None, :]).float() / 4096.0
    ghat = F.normalize(torch.eye(J) + torch.rand(J, J, generator=g) * 0.1, p=1.0, dim=1)
    return x1, x2, W, types, bias, ghat


def _run(dev, route, set_route, x1, x2, W, types, bias, ghat, rms):
    set_route(route)
    B, J, K1 = x1.shape
    N = W.shape[1]
    t = lambda a: None if a is None else a.to(dev).contiguous()  # noqa: E731
    d = {k: t(v) for k, v in dict(x1=x1, x2=x2, W=W, bias=bias, ghat=ghat).items()}
    out = torch.full((B, J, N), float("nan"), device=dev)
    nt = (ctypes.c_int64 * J)(*types.tolist())
    p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    _lib.check(_lib.lib().sd_test_graph_linear_layout(p(d["x1"]), K1, 1, p(d["x2"]), 0 if x2 is None else x2.shape[2],
                                                      p(d["W"]), p(d["bias"]), nt, p(d["ghat"]), None, 0, None,
                                                      out.data_ptr(), B, J, N, int(rms), 0, 0))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("J,nty,K1,K2,N,rms", SHAPES)
@pytest.mark.parametrize("B", ROWS)
def test_direct_store_routes_equal_one_kernel(J, nty, K1, K2, N, rms, B, split_route, cuda):
    args = _inputs(J, nty, K1, K2, N, B)
    ref = _run(cuda, 1, split_route, *args, rms)
    assert torch.isfinite(ref).all()
    # the reference is right (not merely equal): float64 restatement, the kernel tests' 2e-5
    x1, x2, W, types, bias, ghat = args
    x = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    y = torch.einsum("jnk,bjk->bjn", W[types].double(), x.double())
    if rms:
        y = y / x1.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    z = ghat.double() @ (y + bias[types].double())
    assert (ref.double() - z).abs().max().item() < 2e-5 * max(1.0, float(z.abs().max()))
    for route in (3, 2):
        got = _run(cuda, route, split_route, *args, rms)
        assert torch.equal(got, ref), (route, float((got - ref).abs().max()))


@pytest.mark.parametrize("J,nty,K1,K2,N,rms", [(16, 10, 192, 0, 192, False), (16, 10, 192, 192, 192, False),
                                              (16, 10, 192, 0, 768, True)])
@pytest.mark.parametrize("B", ROWS)
def test_direct_store_range_fallback_equals_one_kernel(J, nty, K1, K2, N, rms, B, split_route, cuda):
    """x at 7e4 (>= 65,504: its f16 hi term would be inf) in the last live row -- the single live row
    of the ragged tile: the waves holding it recompute their tiles on exact-f32 MFMA with the
    operands swapped and store them through the same direct path.

    `every`: the element in every node and every 32-row tile, so that each wave of each route
    recomputes all of its tiles and the three routes run the same arithmetic everywhere: routes 2
    and 3 equal route 1 bit for bit.
    One element alone (node 5): a one-kernel wave (route 1) owns several nodes and row tiles and
    recomputes all of them, a GEMM-phase wave its own (row tile, node) only, so route 1 runs
    exact-f32 products where routes 2 and 3 keep the split-f16 ones (measured on the library before
    this change too: 7.6e-6 at |z| = 40, 1.2e-7 with rms).  There routes 2 and 3 -- the same fallback
    granularity -- equal each other bit for bit, and route 1 within the 2e-5 (relative to the row's
    magnitude) of tests/test_gpu_kernels.py::test_graph_linear_out_of_f16_range."""
    for every in (True, False):
        x1, x2, W, types, bias, ghat = _inputs(J, nty, K1, K2, N, B)
        xs = x2 if x2 is not None else x1
        if every:
            xs[31::32, :, 11] = 7e4
            xs[B - 1, :, 11] = 7e4
        else:
            xs[B - 1, 5, 11] = 7e4
        ref = _run(cuda, 1, split_route, x1, x2, W, types, bias, ghat, rms)
        assert torch.isfinite(ref).all()
        got = {route: _run(cuda, route, split_route, x1, x2, W, types, bias, ghat, rms) for route in (3, 2)}
        for route in (3, 2):
            print(f"every={every} route {route}: max |route - route 1| = {float((got[route] - ref).abs().max()):.3e}")
        assert torch.equal(got[3], got[2])
        if every:
            assert torch.equal(got[3], ref) and torch.equal(got[2], ref)
        else:
            scale = ref.abs().amax(dim=(1, 2)).clamp_min(1.0)
            assert float(((got[3] - ref).abs().amax(dim=(1, 2)) / scale).max()) < 2e-5


def _config(name, cuda, rows_factors, T=2):
    from bench import build_config

    batch, futures = rows_factors
    d, x_cond, rows = build_config(name, cuda, T=T, batch=batch, futures=futures)
    assert rows == 33
    return d, x_cond, rows


def test_direct_store_paired_block_range_fallback(cuda):
    """The paired final block at 33 rows with |r| forced out of the f16 range (as
    tests/test_gpu_final_pair.py does): the second half's unscale, f32 weights and bias through the
    swapped exact tile; equal to the one-kernel route, status flag set on both."""
    d, x_cond, rows = _config("amass16", cuda, (3, 11))
    J, D = d.channels, d.seq_length
    big = x_cond * 3e6
    start = torch.from_numpy(O.philox_normal(7, torch.arange(rows).numpy(), 1, J * D).reshape(rows, J, D)).float()
    eng = d.engine
    eng.set_option("row_chains", 1)
    out = {}
    for route in (1, 3, 2):
        eng.set_option("split_route", route)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out[route] = eng.sample_loop(rows, x_cond=big, start_noise=start.to(cuda), graph=False)[0].clone()
            torch.cuda.synchronize()
        assert eng.status(rows) & _lib.SD_STATUS_F16_RANGE, route
    assert torch.isfinite(out[1]).all()
    assert torch.equal(out[3], out[1]) and torch.equal(out[2], out[1])


@pytest.mark.parametrize("cfg,factors,prec", [("amass16", (3, 11), "half"), ("freeman17", (3, 11), "bf16")])
def test_direct_store_half_and_bf16(cfg, factors, prec, cuda):
    """Half (one f16 product) and bf16 operands at 33 rows: the tiled route equals the one-kernel
    route, the equalities tests/test_gpu_configs.py claims at larger batches."""
    d, x_cond, rows = _config(cfg, cuda, factors)
    eng = d.engine
    eng.set_precision(prec)
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = eng.sample_loop(rows, x_cond=x_cond, seed=13, record=(False, True))
    ref = [ref[0].clone(), ref[4].clone()]
    eng.set_option("split_route", 3)
    got = eng.sample_loop(rows, x_cond=x_cond, seed=13, record=(False, True))
    torch.cuda.synchronize()
    assert eng.get_option("last_route") & 8  # k_gl4t ran
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[4], ref[1])
    assert eng.status(rows) == 0


def test_direct_store_rowmajor_chain_matches_oracle(cuda):
    """mano51 (J = 51: v5, whose GEMM phase is k_gl4t / k_gl4y writing row-major z, rows < B only)
    at 33 rows, T = 2: the whole chain against the oracle at the project's 1e-4.  (No plan option
    forces k_gl4y against k_gl4t on this path: launch_gemm_split picks by shape and alignment.)"""
    d, x_cond, rows = _config("mano51", cuda, (3, 11))
    J, D, T = d.channels, d.seq_length, d.num_timesteps
    eng, seed = d.engine, 20261020
    img = eng.sample_loop(rows, x_cond=x_cond, seed=seed, graph=False)[0].clone()
    torch.cuda.synchronize()
    assert eng.status(rows) == 0 and torch.isfinite(img).all()
    sd = {k: v.detach().cpu() for k, v in d.state_dict().items()}
    cfg = O.release_config(J, d.model.node_types)
    bufs = {k: v for k, v in sd.items() if not k.startswith("model.")}
    sel = np.arange(rows)
    normals = lambda step: torch.from_numpy(O.philox_normal(seed, sel, step, J * D).reshape(rows, J, D))  # noqa: E731
    xc = x_cond.cpu().repeat_interleave(rows // x_cond.shape[0], 0)
    x = normals(T)
    for t in range(T - 1, -1, -1):
        x, _ = O.p_sample_step(sd, cfg, bufs, x, t, normals(t), x_cond=xc)
    assert float((img.cpu() - x).abs().max()) < 1e-4
