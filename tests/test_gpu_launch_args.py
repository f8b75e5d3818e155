"""The split route on its compact argument blocks and division-free work-unit decode (DESIGN.md
§4v): k_gl4y, k_gl4t, the mixing phase k_gl4m (MODE 2 / 3) and k_gl4_pair at the shapes where the
decode can go wrong -- grids that are no multiple of 8, a last RT = 2 row group with one live row and
dead tiles, chains that start inside a sequence -- must equal the one-kernel route bit for bit and the
CPU oracle at the project's 1e-4 parity bar.  Release architecture, T = 2.

Rows 33 / 257 / 321 are no multiple of 50 and the engine wants whole sequences, so the sequences hold
11 / 257 / 107 futures (3, 1 and 3 sequences): every chain but the first starts inside a sequence
(x1_row0 != 0), the conditioning-row division (x1_div = futures) stays on the row-major init_lin."""
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = {33: (3, 11), 257: (1, 257), 321: (3, 107)}  # rows: (sequences, futures)
CONFIGS = ["amass16", "freeman17", "amass21"]         # J = 16, 17, 21


def _oracle_blocks(d, x, t, xc):
    """oracle.denoiser_forward with every block output kept (sd_denoiser_trace's list)."""
    sd = {k: v.detach().cpu() for k, v in d.state_dict().items()}
    cfg = O.release_config(d.channels, d.model.node_types)
    net = O.skeldiff_oracle._Net(sd, cfg, "model.")
    h = net.graph_linear("init_lin", torch.cat([xc, x], dim=-1))
    r = h.clone()
    acts = [h]
    tt = torch.full((x.shape[0],), t, dtype=torch.long)
    temb = O.skeldiff_oracle.sinusoidal_embedding(tt, cfg.dim + cfg.cond_dim, cfg.theta).to(h.dtype)
    temb = net.linear("time_mlp.3", torch.nn.functional.gelu(net.linear("time_mlp.1", temb)))
    for i in range(2 * cfg.depth):
        h = net.resnet(f"layers.{i}.0", h, temb)
        acts.append(h)
        if net.has(f"layers.{i}.1.fn.norm.g"):
            h = net.attention(f"layers.{i}.1", h)
        acts.append(h)
    h = net.resnet("final_res_block", torch.cat((h, r), dim=-1), temb)
    acts.append(h)
    return net.graph_linear("final_glin", h), acts


@pytest.mark.parametrize("rows", sorted(SHAPES))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_routes_and_chains_bitwise(cfg, rows, cuda):
    from bench import build_config

    batch, futures = SHAPES[rows]
    d, x_cond, n = build_config(cfg, cuda, T=2, batch=batch, futures=futures)
    assert n == rows
    eng = d.engine
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = eng.sample_loop(rows, x_cond=x_cond, seed=41, record=(False, True))
    ref = [ref[0].clone(), ref[4].clone()]
    assert not eng.get_option("last_route") & (4 | 8 | 16)
    tiles = (rows + 31) // 32
    for route, bit in ((2, 4), (3, 8), (0, 0)):
        eng.set_option("split_route", route)
        for chains in (1, 2, 3):
            eng.set_option("row_chains", chains)
            for graph in ((False, True) if chains != 2 else (False,)):
                got = eng.sample_loop(rows, x_cond=x_cond, seed=41, graph=graph, record=(False, True))
                torch.cuda.synchronize()
                assert eng.get_option("last_chains") == min(chains, tiles), (route, chains)
                assert torch.equal(got[0], ref[0]) and torch.equal(got[4], ref[1]), (cfg, rows, route, chains, graph)
                bits = eng.get_option("last_route")
                assert bits & 16 and (not bit or bits & bit), (route, bits)  # the mixing phase and the forced GEMM phase ran
    assert eng.status(rows) == 0


@pytest.mark.parametrize("rows", sorted(SHAPES))
@pytest.mark.parametrize("cfg", CONFIGS)
def test_trace_blocks_against_oracle(cfg, rows, cuda):
    from bench import build_config

    batch, futures = SHAPES[rows]
    d, x_cond, _ = build_config(cfg, cuda, T=2, batch=batch, futures=futures)
    J, D = d.channels, d.seq_length
    x = torch.from_numpy(O.philox_normal(43, torch.arange(rows).numpy(), 1, J * D).reshape(rows, J, D)).float()
    xc = x_cond.cpu().repeat_interleave(futures, 0)
    want_x0, want = _oracle_blocks(d, x, 1, xc)
    eng = d.engine
    eng.set_option("row_chains", 1)
    first = None
    for route in (1, 2, 3, 0):
        eng.set_option("split_route", route)
        x0, acts = eng.denoiser_trace(x.to(cuda), 1, x_cond)
        torch.cuda.synchronize()
        assert len(acts) == len(want)
        errs = [float((a.cpu() - w).abs().max()) for a, w in zip(acts, want)] + [float((x0.cpu() - want_x0).abs().max())]
        print(cfg, rows, "route", route, "max |gpu - oracle| per block", " ".join(f"{e:.1e}" for e in errs))
        assert max(errs) < 1e-4, (route, errs)
        if first is None:
            first = [a.clone() for a in acts] + [x0.clone()]
        else:  # the routes agree bit for bit, block by block
            for k, (a, b) in enumerate(zip(acts + [x0], first)):
                assert torch.equal(a, b), (cfg, rows, route, k)


def test_auto_route_1300_rows(cuda):
    """1,300 rows (> the 1,200-row split threshold, no multiple of 256): the auto route -- tiled GEMM
    phase, paired final block, three chains -- against the one-kernel route on one chain."""
    from bench import build_config

    d, x_cond, rows = build_config("amass16", cuda, T=2, batch=26)
    assert rows == 1300
    eng = d.engine
    eng.set_option("row_chains", 1)
    eng.set_option("split_route", 1)
    ref = eng.sample_loop(rows, x_cond=x_cond, seed=47, record=(False, True))
    ref = [ref[0].clone(), ref[4].clone()]
    eng.set_option("row_chains", 0)
    eng.set_option("split_route", 0)
    for graph in (False, True):
        got = eng.sample_loop(rows, x_cond=x_cond, seed=47, graph=graph, record=(False, True))
        torch.cuda.synchronize()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[4], ref[1]), graph
    bits = eng.get_option("last_route")
    assert bits & 8 and bits & 16, bits  # the tiled GEMM phase k_gl4t + the mixing phase
    assert eng.status(rows) == 0
