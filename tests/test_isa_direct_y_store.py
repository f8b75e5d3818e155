"""CPU guard of k_gl4t's store tail: Y goes from the swapped-operand MFMA
accumulators straight to memory.  After the K loop's last s_barrier and outside the f16-range
fallback loop, the shipped code objects of the two k_gl4t forms tests/test_isa_waits.py names hold
no LDS write (no transpose), no further barrier, and no global store narrower than dwordx4."""
import re

import pytest

from test_isa_waits import GL4T, GL4T_RT2, _disasm, pytestmark  # noqa: F401



def _tail(ins):
    """Instructions from the last s_barrier to s_endpgm.  The f16-range fallback loops are left in:
    they store through the same direct path, so the three properties hold for them too (a stronger
    check than one that cuts them out)."""
    last_barrier = max(i for i, l in enumerate(ins) if l.startswith("s_barrier"))
    end = max(i for i, l in enumerate(ins) if l.startswith("s_endpgm"))
    tail = ins[last_barrier + 1:end + 1]
    return tail


@pytest.mark.parametrize("sym,normal_stores", [(GL4T, 24), (GL4T_RT2, 24)])
def test_gl4t_tail_stores_from_registers(sym, normal_stores, tmp_path_factory):
    ins = _disasm(tmp_path_factory, sym)
    tail = _tail(ins)
    # no transpose and no barrier anywhere behind the K loop, the fallback included (it stores
    # through the same direct path)
    assert not any(l.startswith("s_barrier") for l in tail)
    assert not any(l.startswith("ds_write") for l in tail), [l for l in tail if l.startswith("ds_write")][:4]
    stores = [l for l in tail if l.startswith("global_store")]
    narrow = [l for l in stores if not l.startswith("global_store_dwordx4")]
    assert narrow == [], narrow[:4]
    # the normal tail: 4 dwordx4 per tile (6 tiles, RT x CT) + the fallback's 4 per row tile
    assert len(stores) >= normal_stores, len(stores)
    # the bias comes back from LDS as 16-B pieces
    assert any(l.startswith("ds_read_b128") for l in tail)
