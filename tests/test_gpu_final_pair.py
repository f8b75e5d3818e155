"""final_res_block's res_linear and block1 as one paired launch per phase.

Both layers read cat(x, r); on the tiled split route (k_gl4t + MODE 2) their GEMM phases run as
one k_gl4t launch over 2 N columns and their mixing phases as one launch over both layers' column
tiles.  Per accumulator element nothing changes, so the results must equal the one-kernel route
(SD_OPT_SPLIT_ROUTE 1, never paired) bit for bit: final latents and every per-step record, eager
and graph, on one row chain and on three."""
import warnings

import pytest
import torch

import oracle as O
from skeletondiffusion_amd import _lib

pytestmark = pytest.mark.gpu

# (config, sequences, futures, precision): 40 rows = one full 32-row tile + a ragged one (an RT = 2
# wave holds a live and a ragged tile), 300 rows = a ragged 256-row group, J = 17 / 21 at 80 rows,
# the half and bf16 forms of the GEMM phase
CASES = [("amass16", 8, 5, "f32"), ("amass16", 6, 50, "f32"), ("freeman17", 16, 5, "f32"), ("amass21", 16, 5, "f32"),
         ("amass16", 8, 5, "half"), ("freeman17", 16, 5, "bf16")]


def _launches(d, x_cond, rows):
    """graph-linear launches of one denoiser step (sd_profile_step: a paired launch counts once)"""
    from bench import profile_kernels

    return profile_kernels(d, x_cond, rows, reps=1)[1][0]


@pytest.mark.parametrize("cfg,batch,futures,prec", CASES)
def test_final_pair_bitwise(cfg, batch, futures, prec, cuda):
    from bench import build_config

    d, x_cond, rows = build_config(cfg, cuda, T=3, batch=batch, futures=futures)
    eng = d.engine
    eng.set_precision(prec)
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = eng.sample_loop(rows, x_cond=x_cond, seed=31, record=(False, True))
    ref = [ref[0].clone(), ref[4].clone()]
    assert not eng.get_option("last_route") & 8
    n1 = _launches(d, x_cond, rows)
    eng.set_option("split_route", 3)
    for chains in (1, 3):
        eng.set_option("row_chains", chains)
        for graph in (False, True):
            got = eng.sample_loop(rows, x_cond=x_cond, seed=31, graph=graph, record=(False, True))
            torch.cuda.synchronize()
            assert eng.get_option("last_chains") == min(chains, (rows + 31) // 32)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[4], ref[1]), (cfg, prec, chains, graph)
            bits = eng.get_option("last_route")
            assert bits & 8 and bits & 16, bits  # k_gl4t GEMM phase + MODE 2 / 3 mixing phase
    assert eng.status(rows) == 0
    # the pair ran: one graph-linear launch fewer per step than layer by layer
    assert _launches(d, x_cond, rows) == n1 - 1


def test_final_pair_f16_range_guard(cuda):
    """Conditioning latents scaled until r = init_lin(cat(x_cond, x)) -- no activation, so it reaches
    the final block's input as it is -- leaves the f16 range (|r| >= 65,504): the paired GEMM phase
    recomputes the affected tiles on exact-f32 MFMA with each half's own weights, scale and bias,
    sets the status bit, and still equals the one-kernel route bit for bit."""
    from bench import build_config

    d, x_cond, rows = build_config("amass16", cuda, T=1, batch=8, futures=5)
    J, D = d.channels, d.seq_length
    big = x_cond * 3e6
    start = torch.from_numpy(O.philox_normal(7, torch.arange(rows).numpy(), 1, J * D).reshape(rows, J, D)).float()
    # CPU oracle: the scaled input does leave the range, and the latents stay finite
    sd = {k: v.detach().cpu() for k, v in d.state_dict().items()}
    cfg = O.release_config(J, d.model.node_types)
    bufs = {k: v for k, v in sd.items() if not k.startswith("model.")}
    xc = big.cpu().repeat_interleave(rows // big.shape[0], 0)
    r = O.skeldiff_oracle._Net(sd, cfg, "model.").graph_linear("init_lin", torch.cat([xc, start], dim=-1))
    assert float(r.abs().max()) > 65504.0
    img, _ = O.p_sample_loop(sd, cfg, bufs, start, torch.zeros((rows, 0, J, D)), x_cond=xc)
    assert torch.isfinite(img).all()
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
    assert torch.isfinite(out[3]).all()
    assert torch.equal(out[1], out[3])
