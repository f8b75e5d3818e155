"""The GEMM phase's Y stores go through sd::store16 with the write-through policy (sd_store_policy.h,
DESIGN.md §4ab): k_gl4t (route 3) and k_gl4y (route 2) write every scratch block with 16-B stores
that carry the sc1 bit, not tracked by the compiler's wait counting.  A store policy changes where the
bytes sit between two kernels, never which bytes: every result must stay bit for bit what the
one-kernel route (route 1, which has no Y in memory at all) computes, on one chain and on three
(another chain's kernels run beside the boundary), eager and as a captured graph.

Rows: 33 (a ragged 32-row tile: one live row in the second), 257 (a ragged 256-row group, dead
tiles in the last workgroup), 1,300 (above the split threshold: the tiled route by auto, the paired
final block, three chains).  33 / 257 rows are 3 sequences of 11 futures / 1 of 257, so chains start
inside a sequence.  J = 16 and 17, f32 (three f16 products), half and bf16.

A visibility bug of such a store shows as wrong rows, not as a fault: these equalities are the
detector."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

import oracle as O
from skeletondiffusion_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = {33: (3, 11), 257: (1, 257), 1300: (26, 50)}  # rows: (sequences, futures)
CONFIGS = ["amass16", "freeman17"]                     # J = 16, 17
PRECISIONS = ["f32", "half", "bf16"]
T = 3
# where a forced split route exists (split_route, sd_graph_linear_v4.hip): everywhere but route 2 in bf16
# mode (k_gl4y has no bf16 form: the one-kernel tiles run, and the equalities hold on them)
FORCED = {(c, p, r) for c in CONFIGS for p in PRECISIONS for r in (2, 3) if (p, r) != ("bf16", 2)}


def _build(cfg, rows, cuda, prec="f32"):
    from bench import build_config

    batch, futures = SHAPES[rows]
    d, x_cond, n = build_config(cfg, cuda, T=T, batch=batch, futures=futures)
    assert n == rows
    d.engine.set_precision(prec)
    return d, x_cond


def _sample(eng, rows, x_cond, graph=False):
    got = eng.sample_loop(rows, x_cond=x_cond, seed=53, graph=graph, record=(False, True))
    torch.cuda.synchronize()
    return [got[0].clone(), got[4].clone()]  # the latents and every step's x_t


def _forward(d, rows, x_cond, cuda):
    J, D = d.channels, d.seq_length
    x = torch.from_numpy(O.philox_normal(59, torch.arange(rows).numpy(), 1, J * D).reshape(rows, J, D)).float()
    x0 = d.engine.denoiser_forward(x.to(cuda), 1, x_cond)
    torch.cuda.synchronize()
    return x0.clone()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("rows", [33, 257])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_forced_split_routes_equal_one_kernel(cfg, rows, prec, cuda):
    d, x_cond = _build(cfg, rows, cuda, prec)
    eng = d.engine
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = _sample(eng, rows, x_cond)
    assert not eng.get_option("last_route") & (4 | 8 | 16)  # no GEMM phase, no mixing phase: the one-kernel route
    assert all(torch.isfinite(t).all() for t in ref)
    ref_fwd = _forward(d, rows, x_cond, cuda)
    tiles = (rows + 31) // 32
    for route, bit in ((3, 8), (2, 4)):
        eng.set_option("split_route", route)
        eng.set_option("row_chains", 1)
        assert torch.equal(_forward(d, rows, x_cond, cuda), ref_fwd), (cfg, rows, prec, route)  # one denoiser forward
        for chains in (1, 3):
            eng.set_option("row_chains", chains)
            for graph in (False, True):
                got = _sample(eng, rows, x_cond, graph)
                assert eng.get_option("last_chains") == min(chains, tiles)
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (cfg, rows, prec, route, chains, graph)
                bits = eng.get_option("last_route")
                print(cfg, rows, prec, "route", route, "chains", chains, "graph", graph, "route bits", bits)
                if (cfg, prec, route) in FORCED:  # the forced GEMM phase and the mixing phase ran: Y went through memory
                    assert bits & 16 and bits & bit, (route, bits)
    assert eng.status(rows) == 0


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_auto_route_1300_rows_equals_one_kernel(cfg, prec, cuda):
    """Auto route, then the tiled route forced: J = 16 in half / bf16 keeps the one-kernel tiles by auto at
    full batches, so only the forced pass runs the write-through stores there."""
    rows = 1300
    d, x_cond = _build(cfg, rows, cuda, prec)
    eng = d.engine
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = _sample(eng, rows, x_cond)
    ref_fwd = _forward(d, rows, x_cond, cuda)
    assert all(torch.isfinite(t).all() for t in ref)
    for route in (0, 3):
        eng.set_option("split_route", route)
        eng.set_option("row_chains", 1)
        assert torch.equal(_forward(d, rows, x_cond, cuda), ref_fwd), (cfg, prec, route)
        for chains in (1, 3):
            eng.set_option("row_chains", chains)
            for graph in (False, True):
                got = _sample(eng, rows, x_cond, graph)
                assert eng.get_option("last_chains") == chains
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (cfg, prec, route, chains, graph)
        bits = eng.get_option("last_route")
        print(cfg, prec, "route", route, "route bits", bits)
        if route == 3 or prec == "f32" or cfg == "freeman17":
            assert bits & 8 and bits & 16, bits  # the tiled GEMM phase k_gl4t + the mixing phase
    assert eng.status(rows) == 0


def _layer(dev, route, x1, W, types, bias, ghat):
    L = _lib.lib()
    assert L.sd_test_set_split_route(route) >= 0
    try:
        B, J, K1 = x1.shape
        N = W.shape[1]
        d = {k: v.to(dev).contiguous() for k, v in dict(x1=x1, W=W, bias=bias, ghat=ghat).items()}
        out = torch.full((B, J, N), float("nan"), device=dev)
        nt = (ctypes.c_int64 * J)(*types.tolist())
        _lib.check(L.sd_test_graph_linear_layout(d["x1"].data_ptr(), K1, 1, None, 0, d["W"].data_ptr(), d["bias"].data_ptr(), nt,
                                                 d["ghat"].data_ptr(), None, 0, None, out.data_ptr(), B, J, N, 0, 0, 0))
        torch.cuda.synchronize()
    finally:
        L.sd_test_set_split_route(0)
    return out.cpu()


@pytest.mark.parametrize("N", [192, 768])
def test_range_fallback_second_store_wins(N, cuda):
    """64 rows, the tiled route forced, one input element at 7e4 (>= 65,504: its f16 hi term is inf).
    The wave that holds it stores its tiles twice -- the split-f16 tile (inf - inf: NaN), then the
    exact-f32 tile over it, same lanes, same addresses, both through the same store helper.  The
    scratch must hold the second: every output finite and within the kernel tests' 2e-5 (relative to
    max |z|) of the float64 restatement; k_gl4y (route 2) runs the same fallback at the same
    granularity and must agree bit for bit."""
    B, J, nty, K = 64, 16, 10, 192
    g = torch.Generator().manual_seed(6400 + N)
    x1 = torch.rand(B, J, K, generator=g) * 2 - 1
    x1[B - 1, 5, 11] = 7e4
    W = (torch.rand(nty, N, K, generator=g) * 2 - 1) / K ** 0.5
    types = torch.arange(J) % nty
    bias = (1000.0 * torch.arange(nty)[:, None] + torch.arange(N)[None, :]).float() / 4096.0
    ghat = F.normalize(torch.eye(J) + torch.rand(J, J, generator=g) * 0.1, p=1.0, dim=1)
    got = _layer(cuda, 3, x1, W, types, bias, ghat)
    assert torch.isfinite(got).all()
    z = ghat.double() @ (torch.einsum("jnk,bjk->bjn", W[types].double(), x1.double()) + bias[types].double())
    err = float((got.double() - z).abs().max())
    print(f"N = {N}: max |route 3 - f64| = {err:.3e} at max |z| = {float(z.abs().max()):.3e}")
    assert err < 2e-5 * max(1.0, float(z.abs().max()))
    assert torch.equal(_layer(cuda, 2, x1, W, types, bias, ghat), got)


def test_range_fallback_sets_status(cuda):
    """The whole chain at 64 rows with the conditioning out of the f16 range: the tiled route stores
    its tiles twice in every layer that sees it, equals the one-kernel route and raises the status bit."""
    from bench import build_config

    d, x_cond, rows = build_config("amass16", cuda, T=T, batch=2, futures=32)
    assert rows == 64
    J, D = d.channels, d.seq_length
    big = x_cond * 3e6
    start = torch.from_numpy(O.philox_normal(7, torch.arange(rows).numpy(), 1, J * D).reshape(rows, J, D)).float()
    eng = d.engine
    eng.set_option("row_chains", 1)
    out = {}
    for route in (1, 3):
        eng.set_option("split_route", route)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out[route] = eng.sample_loop(rows, x_cond=big, start_noise=start.to(cuda), graph=False)[0].clone()
            torch.cuda.synchronize()
        assert eng.status(rows) & _lib.SD_STATUS_F16_RANGE, route
    assert eng.get_option("last_route") & 8
    assert torch.isfinite(out[1]).all()
    assert torch.equal(out[3], out[1])


@pytest.mark.parametrize("rows,factors", [(33, (3, 11)), (1024, (32, 32))])
def test_update_mfma_equals_elementwise(rows, factors, cuda):
    """k_update_mfma (its x_{t-1} stores stay plain: one instruction writes 64 B to each of 16 lines)
    against the element-per-thread forms, latents, records and every x_t, bit for bit."""
    from bench import build_config

    d, x_cond, n = build_config("amass16", cuda, T=T, batch=factors[0], futures=factors[1])
    assert n == rows
    eng = d.engine
    res = {}
    for v in (1, 0):  # 1 the element-per-thread forms, 0 (default) k_update_mfma
        eng.set_option("update_kernel", v)
        a = eng.sample_loop(rows, x_cond=x_cond, seed=4, record=(True, False), graph=False)
        b = eng.sample_loop(rows, x_cond=x_cond, seed=4, record=(False, True), graph=False)
        torch.cuda.synchronize()
        res[v] = [t.clone() for t in (a[0], a[1], a[2], a[3], b[4])]  # img, start, noise_t, mean_t, imgs
    for name, x, y in zip(("img", "start", "noise_t", "mean_t", "imgs"), res[0], res[1]):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
