"""Row chains cut on the tiled route's GEMM row group compute what one chain
computes: 1,650 rows (33 sequences x 50 futures, not a multiple of 32) on the default route --
the tiled split route, whose chains start on sd_chain_tile_unit rows here (3 chains of at least
512 rows) -- in graph and eager mode."""
import pytest
import torch

from skeletondiffusion_amd import _lib

pytestmark = pytest.mark.gpu


def test_tile_cut_chains_bitwise(cuda):
    from bench import build_config

    d, x_cond, rows = build_config("amass16", cuda, T=2, batch=33)
    assert rows == 1650
    lib = _lib.lib()
    unit = lib.sd_chain_tile_unit()
    # the tile rule applies to both chain counts at this size (and moves the cuts off the 32-row ones)
    for n in (3, 2):
        s = [lib.sd_chain_start(rows, n, unit, i) for i in range(n + 1)]
        assert all(b - a >= 512 for a, b in zip(s, s[1:])) and all(x % unit == 0 for x in s[:n]), s
    assert [lib.sd_chain_start(rows, 3, unit, i) for i in range(4)] != [lib.sd_chain_start(rows, 3, 32, i) for i in range(4)]
    eng = d.engine
    eng.set_option("row_chains", 1)
    ref = eng.sample_loop(rows, x_cond=x_cond, seed=29, record=(False, True))
    ref = [ref[0].clone(), ref[4].clone()]
    assert eng.get_option("last_chains") == 1
    for n in (3, 2):
        eng.set_option("row_chains", n)
        for graph in (True, False):
            got = eng.sample_loop(rows, x_cond=x_cond, seed=29, graph=graph, record=(False, True))
            torch.cuda.synchronize()
            assert eng.get_option("last_chains") == n
            assert torch.equal(got[0], ref[0]) and torch.equal(got[4], ref[1]), (n, graph)
    bits = eng.get_option("last_route")
    assert bits & 8 and bits & 16, bits  # the tiled route: k_gl4t GEMM phase + mixing phase
    assert eng.status(rows) == 0
