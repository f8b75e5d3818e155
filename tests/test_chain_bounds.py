"""Row-chain boundaries (sd_chain_start): host arithmetic, no device.

A sampling call on the tiled split route cuts its row chains on the GEMM phase's row group
(sd_chain_tile_unit rows) where every chain keeps at least two full 256-row workgroups, and on
32-row blocks -- the rule of every earlier round -- everywhere else."""
from skeletondiffusion_amd import _lib


def parent_start(rows, n, i):
    """the 32-row rule: chain i of n starts at ceil(rows / 32) * i / n * 32"""
    return rows if i >= n else min(rows, (rows + 31) // 32 * i // n * 32)


def starts(lib, rows, n, unit):
    return [lib.sd_chain_start(rows, n, unit, i) for i in range(n + 1)]


def test_tile_unit_is_a_gemm_row_group():
    unit = _lib.lib().sd_chain_tile_unit()
    assert unit in (64, 128, 256)  # one RT = 2 wave, one to_qkv workgroup, one k_gl4t workgroup


def test_chain_starts_partition_the_rows():
    lib = _lib.lib()
    unit = lib.sd_chain_tile_unit()
    applied = 0
    for rows in range(1, 4001):
        for n in (1, 2, 3):
            s = starts(lib, rows, n, unit)
            assert s[0] == 0 and s[n] == rows, (rows, n, s)
            assert all(a <= b for a, b in zip(s, s[1:])), (rows, n, s)
            assert all(x % 32 == 0 for x in s[:n]), (rows, n, s)
            # sd_sample_loop never asks for more chains than 32-row units (chain_count): there every
            # chain holds rows
            if (rows + 31) // 32 >= n:
                assert all(a < b for a, b in zip(s, s[1:])), (rows, n, s)
            par = [parent_start(rows, n, i) for i in range(n + 1)]
            # the rule applies where the cuts on `unit` rows leave every chain 512 rows
            cut = [rows if i >= n else min(rows, (rows + unit - 1) // unit * i // n * unit) for i in range(n + 1)]
            if all(b - a >= 512 for a, b in zip(cut, cut[1:])):
                assert s == cut and all(x % unit == 0 for x in s[:n]), (rows, n, s)
                applied += 1
            else:
                assert s == par, (rows, n, s, par)
            # the 32-row rule itself (any call off the tiled route)
            assert starts(lib, rows, n, 32) == par
    assert applied > 0


def test_headline_split():
    """config 2: 3,200 rows on three chains"""
    lib = _lib.lib()
    assert starts(lib, 3200, 3, 32) == [0, 1056, 2112, 3200]
    assert starts(lib, 3200, 3, 64) == [0, 1024, 2112, 3200]
    assert starts(lib, 3200, 3, 128) == [0, 1024, 2048, 3200]
    assert starts(lib, 3200, 3, 256) == [0, 1024, 2048, 3200]
    # 1,500 rows: 128-row cuts would leave 512 + 512 + 476, so the 32-row cuts stay
    assert starts(lib, 1500, 3, 128) == [parent_start(1500, 3, i) for i in range(4)]
