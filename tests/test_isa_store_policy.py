"""CPU guard of the store policy (sd_store_policy.h) on the shipped code objects:
every k_gl4t, k_gl4y, k_gl4m, k_gl4_pair and k_update_mfma symbol of the built libskeldiff.so.

* no scratch anywhere (the metadata's private segment is 0 and no scratch_ instruction);
* the GEMM phase's stores into the row-blocked scratch (k_gl4t and k_gl4y with ROWMAJOR = false) all
  carry the write-through bit sc1; the row-major forms (the J > 21 path), the mixing and attention
  phases (k_gl4m, k_gl4_pair) and the posterior update (k_update_mfma) carry it nowhere -- one store
  instruction of theirs writes parts of lines;
* the number of 16-B global stores per symbol is what it was before the policy (recorded below): the
  helper adds no store and splits none.
"""
import os
import re
import subprocess

import pytest

from skeletondiffusion_amd import isa_check
from test_isa_waits import LIB, OBJDUMP, _objects, pytestmark  # noqa: F401

GL4T = re.compile(r"6k_gl4tILb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELi(\d+)EEE")  # RMS PREC CT NCH ROWMAJOR RT PF
GL4Y = re.compile(r"6k_gl4yILb([01])ELi(\d+)ELb([01])ELi(\d+)EEE")                           # RMS PREC ROWMAJOR PF
OTHER = re.compile(r"(6k_gl4mI|10k_gl4_pairI|13k_update_mfmaI)((?:L[ib]\d+E)+)E")

# 16-B global stores per symbol before the policy.
# k_gl4t: 4 per 32 x 32 tile, RT x CT tiles, + per row tile the rolled range-fallback loop's 4 (no
# fallback with bf16 operands, PREC 2); k_gl4y: 4 + the fallback's 4.
# The others by template arguments: k_gl4m<J, MODE, PREC>, k_gl4_pair<J, PREC>, k_update_mfma<JP, R, MT, BF>.
STORES_BEFORE = {
    "k_gl4m": {(16, 2, 0): 4, (16, 2, 2): 4, (16, 3, 0): 8, (16, 3, 2): 8, (17, 2, 0): 8, (17, 2, 2): 8, (17, 3, 0): 16,
               (17, 3, 2): 16, (21, 2, 0): 8, (21, 2, 2): 8, (21, 3, 0): 16, (21, 3, 2): 16},
    "k_gl4_pair": {(16, 0): 8, (16, 2): 8, (17, 0): 16, (17, 2): 16, (21, 0): 16, (21, 2): 16},
    "k_update_mfma": {(16, 1, 2, 0): 33, (16, 1, 2, 1): 33, (16, 4, 6, 0): 45, (16, 4, 6, 1): 45, (32, 1, 2, 0): 39,
                      (32, 1, 2, 1): 39, (32, 4, 6, 0): 63, (32, 4, 6, 1): 63, (64, 1, 2, 0): 51, (64, 1, 2, 1): 51},
}

_cache = {}


def _symbols(tmp_path_factory):
    """{symbol: instructions} of the five kernel families, one objdump call per code object."""
    if "syms" in _cache:
        return _cache["syms"]
    names = sorted(n for n in isa_check.resources(LIB) if GL4T.search(n) or GL4Y.search(n) or OTHER.search(n))
    assert names
    out = {}
    for path in _objects(str(tmp_path_factory.getbasetemp())):
        txt = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", "--disassemble-symbols=" + ",".join(names), path],
                             capture_output=True, text=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            line = line.split("//")[0].strip()
            if cur is not None and line:
                cur.append(line)
    out = {k: v for k, v in out.items() if any(l.startswith("s_endpgm") for l in v)}
    assert sorted(out) == names, sorted(set(names) - set(out))
    _cache["syms"] = out
    return out


def _stores16(ins):
    return [l for l in ins if l.startswith("global_store_dwordx4")]


def _targs(s):
    return tuple(int(x) for x in re.findall(r"L[ib](\d+)E", s))


def test_no_scratch(tmp_path_factory):
    res = isa_check.resources(LIB)
    for sym, ins in _symbols(tmp_path_factory).items():
        assert res[sym]["private_segment_fixed_size"] == 0 and res[sym].get("vgpr_spill_count", 0) == 0, sym
        assert not any(l.startswith("scratch_") for l in ins), sym


def test_gemm_phase_scratch_stores_write_through(tmp_path_factory):
    seen = {True: 0, False: 0}
    for sym, ins in _symbols(tmp_path_factory).items():
        m = GL4T.search(sym) or GL4Y.search(sym)
        if not m:
            continue
        rowmajor = bool(int(m.group(5 if GL4T.search(sym) else 3)))
        st = [l for l in ins if l.startswith("global_store")]
        wt = [l for l in st if re.search(r"\bsc1\b", l)]
        if rowmajor:
            assert wt == [], (sym, wt[:2])
        else:  # every store of the kernel is a Y store: all 16 B, all written through
            assert st and wt == st and st == _stores16(ins), (sym, [l for l in st if l not in wt][:2])
        seen[rowmajor] += 1
    assert seen[True] and seen[False], seen


def test_write_through_stores_carry_their_wait_states(tmp_path_factory):
    """The write-through store is inline asm, so the compiler pads nothing behind it: a VALU instruction
    that overwrites the store's data VGPRs needs two wait states after a dwordx4 store.  The asm string
    ends with `s_nop 1`, so in the code object EVERY sc1 store is directly followed by it, whatever the
    register allocator does with the instructions after."""
    n = 0
    for sym, ins in _symbols(tmp_path_factory).items():
        for i, l in enumerate(ins):
            if l.startswith("global_store") and re.search(r"\bsc1\b", l):
                assert re.match(r"s_nop 1\b", ins[i + 1]), (sym, l, ins[i + 1])
                n += 1
    assert n >= 1000, n  # (1,472 in the library this was written against)


def test_other_phases_store_plain(tmp_path_factory):
    n = 0
    for sym, ins in _symbols(tmp_path_factory).items():
        if OTHER.search(sym):
            wt = [l for l in ins if l.startswith(("global_store", "buffer_store")) and re.search(r"\bsc1\b", l)]
            assert wt == [], (sym, wt[:2])
            n += 1
    assert n


def test_store_counts_unchanged(tmp_path_factory):
    for sym, ins in _symbols(tmp_path_factory).items():
        n = len(_stores16(ins))
        m = GL4T.search(sym)
        if m:
            _rms, prec, ct, _nch, _rm, rt, _pf = (int(x) for x in m.groups())
            assert n == 4 * rt * (ct + (prec != 2)), (sym, n)
            continue
        if GL4Y.search(sym):
            assert n == 8, (sym, n)
            continue
        m = OTHER.search(sym)
        family = {"6k_gl4mI": "k_gl4m", "10k_gl4_pairI": "k_gl4_pair", "13k_update_mfmaI": "k_update_mfma"}[m.group(1)]
        assert n == STORES_BEFORE[family][_targs(m.group(2))], (sym, n)
