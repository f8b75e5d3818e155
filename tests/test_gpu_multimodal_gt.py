"""The multimodal ground truth on the device (multimodal_gt; C entries sd_cdist, sd_set_mean_distance; DESIGN.md
§4q) against float64, against exact integer cases and against tests/golden/mmgt.npz: the reference's own
get_multimodal_gt adjacency, float64 apd table and MetricStorerAPDE value (gen_golden_mmgt.py).

Tolerances.  sd_cdist sums a pair's squared differences in one blocked order (sd_mmgt.hip): chunks of K_CHUNK = 32
features, inside a chunk one fma per feature into a partial that starts at 0, then the partials added in chunk
order.  The longest chain of roundings a term passes through is CHAIN(D) = K_CHUNK + ceil(D / K_CHUNK).  Every
term is non-negative, so the sum's relative error is at most CHAIN(D) u (u = 2^-24, first order), the rounding of
each difference adds 2 u to its square, the square root halves the total and rounds once: well inside the
(CHAIN(D) + 7) u the tests hold the distance to.  The set mean adds float64 terms: nothing visible in float32."""
import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import _lib, metrics, multimodal_gt
from test_multimodal_gt import BATCHES, reference_dict

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
K_CHUNK = 32  # sd_mmgt.hip kKC


def CHAIN(D):
    """Longest sequential chain of roundings in sd_cdist's feature sum: K_CHUNK fma steps inside a chunk, then one
    add per chunk."""
    return K_CHUNK + -(-D // K_CHUNK)


def d64(x, y):
    x, y = x.double().cpu(), y.double().cpu()
    return ((x[:, None] - y[None]) ** 2).sum(-1).sqrt()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("m,n,D", [(70, 131, 48), (1, 1, 1), (64, 64, 51), (5, 300, 4800), (130, 70, 7)])
def test_cdist_against_float64(m, n, D, cuda):
    g = torch.Generator().manual_seed(1000 + D)
    x, y = torch.randn(m, D, generator=g), torch.randn(n, D, generator=g)
    got = multimodal_gt.cdist(x.to(cuda), y.to(cuda))
    assert got.shape == (m, n) and got.dtype == torch.float32
    ref = d64(x, y)
    rel = float(((got.cpu().double() - ref).abs() / ref).max())
    bound = (CHAIN(D) + 7) * U
    print(f"cdist ({m}, {n}, {D}): max relative error {rel:.2e}, bound {bound:.2e}")
    assert rel <= bound


def test_cdist_exact_integers_and_strict_threshold(cuda):
    """Coordinates in {0..3}: every square, sum and root is exact or correctly rounded in float32, so the result
    equals the host expression bitwise; pairs at exactly d = thr are excluded by the strict <."""
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, 4, (70, 48), generator=g).float()
    y = torch.randint(0, 4, (131, 48), generator=g).float()
    d2 = ((x[:, None] - y[None]) ** 2).sum(-1)
    # the correctly rounded float32 root, formed in float64 and rounded once more: the root of an integer is exact or
    # irrational, never a float32 midpoint, so the two roundings agree with one.  (A host library's vectorised
    # float32 sqrt need not round correctly: on the MI355X host it returned 12.124356 for sqrt(147) = 12.12435565...,
    # whose nearest float32 is 12.124355.)
    want = d2.double().sqrt().float()
    got = multimodal_gt.cdist(x.to(cuda), y.to(cuda)).cpu()
    assert torch.equal(bits(got), bits(want))
    thr = 10.0
    ties = d2 == 100
    assert int(ties.sum()) >= 1, "the input must hold a pair at exactly the threshold"
    hits = got < thr
    assert torch.equal(hits, d2 < 100) and not bool(hits[ties].any())


def test_cdist_invariances_are_bitwise(cuda):
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(130, 51, generator=g).to(cuda), torch.randn(70, 51, generator=g).to(cuda)
    # symmetric with a zero diagonal
    s = multimodal_gt.cdist(x, x)
    assert torch.equal(bits(s), bits(s.T)) and not bool(s.diagonal().any())
    # row chunks of 37 give the bits of one call
    whole = multimodal_gt.cdist(x, y)
    parts = torch.cat([multimodal_gt.cdist(x[a:a + 37], y) for a in range(0, 130, 37)])
    assert torch.equal(bits(parts), bits(whole))
    # swapping the operands gives the transpose
    assert torch.equal(bits(multimodal_gt.cdist(y, x)), bits(whole.T))


@pytest.mark.parametrize("m,n,D", [(70, 64, 48), (70, 131, 48)])
def test_cdist_alignment_does_not_change_a_bit(m, n, D, cuda):
    """Inputs and output one float past a 16-byte boundary take the 4-byte paths: the same bits as the aligned call
    (n = 64 with 16-byte stores, n = 131 without)."""
    g = torch.Generator().manual_seed(13)
    x, y = torch.randn(m, D, generator=g).to(cuda), torch.randn(n, D, generator=g).to(cuda)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    whole = multimodal_gt.cdist(x, y)
    assert whole.data_ptr() % 16 == 0

    def shifted(t):
        base = torch.empty(t.numel() + 1, device=cuda)
        v = base[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    assert torch.equal(bits(multimodal_gt.cdist(shifted(x), shifted(y))), bits(whole))
    assert torch.equal(bits(multimodal_gt.cdist(shifted(x), y)), bits(whole))
    out = shifted(torch.zeros(m, n, device=cuda))
    assert torch.equal(bits(multimodal_gt.cdist(x, y, out=out)), bits(whole))


@pytest.mark.parametrize("chunk_rows", [64, 2048])
def test_get_multimodal_gt_equals_the_reference(chunk_rows, cuda):
    z = golden("mmgt")
    last = torch.from_numpy(z["obs"])[:, -1].to(cuda)  # (150, 16, 3)
    g = multimodal_gt.get_multimodal_gt(last, float(z["thr"]), chunk_rows=chunk_rows)
    assert g.row_ptr.device.type == "cuda" and g.row_ptr.dtype == torch.int64 and g.col.dtype == torch.int64
    assert torch.equal(g.row_ptr.cpu(), torch.from_numpy(z["row_ptr"]))
    assert torch.equal(g.col.cpu(), torch.from_numpy(z["col"]))
    assert torch.equal(g.row_ptr_host, torch.from_numpy(z["row_ptr"]))
    assert g.to_dict() == reference_dict(z)
    flat = multimodal_gt.get_multimodal_gt(last.reshape(150, 48), float(z["thr"]), chunk_rows=chunk_rows)
    assert torch.equal(flat.col, g.col)


def fixture_csr(cuda):
    z = golden("mmgt")
    return z, multimodal_gt.MultimodalGT(torch.from_numpy(z["row_ptr"]), torch.from_numpy(z["col"]), cuda)


def test_gt_apd_against_the_reference(cuda):
    z, g = fixture_csr(cuda)
    futures = torch.from_numpy(z["futures"]).to(cuda)
    D = futures[0].numel()
    assert (CHAIN(D) + 7) * U <= 1e-5  # the distances' bound; the float64 set sum adds nothing visible
    got = g.gt_apd(futures)
    assert got.shape == (150,) and got.dtype == torch.float32
    ref = torch.from_numpy(z["gt_apd"])
    sizes = torch.from_numpy(np.diff(z["row_ptr"]))
    many = sizes > 1
    rel = float(((got.cpu().double() - ref)[many].abs() / ref[many]).max())
    print(f"gt_apd: max relative error {rel:.2e}")
    assert rel <= 1e-5
    assert int((~many).sum()) >= 1 and not bool(got.cpu()[~many].any())  # singleton sets: exactly 0


def test_set_mean_distance_by_hand(cuda):
    """Sets {1, 3, 4}, {} and {2} over a 5 x 5 matrix: the mean of the three pairs, NaN, 0."""
    dist = torch.arange(25, dtype=torch.float32).reshape(5, 5).to(cuda)
    row_ptr = torch.tensor([0, 3, 3, 4], dtype=torch.int64, device=cuda)
    col = torch.tensor([1, 3, 4, 2], dtype=torch.int64, device=cuda)
    out = torch.full((3,), -1.0, device=cuda)
    _lib.check(_lib.lib().sd_set_mean_distance(dist.data_ptr(), 5, row_ptr.data_ptr(), col.data_ptr(), 3, out.data_ptr(),
                                               torch.cuda.current_stream(cuda).cuda_stream))
    out = out.cpu()
    assert float(out[0]) == (8.0 + 9.0 + 19.0) / 3 and bool(torch.isnan(out[1])) and float(out[2]) == 0.0


def test_set_mean_distance_on_a_large_set(cuda):
    """300 members: more partners than a wave has lanes and more first members than a workgroup has waves."""
    g = torch.Generator().manual_seed(17)
    n = 300
    dist = torch.rand(n, n, generator=g)
    perm = torch.randperm(n, generator=g)
    row_ptr = torch.tensor([0, n], dtype=torch.int64, device=cuda)
    out = torch.empty(1, device=cuda)
    d, col = dist.to(cuda), perm.to(cuda)
    _lib.check(_lib.lib().sd_set_mean_distance(d.data_ptr(), n, row_ptr.data_ptr(), col.data_ptr(), 1,
                                               out.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream))
    sub = dist[perm][:, perm].double()
    iu = torch.triu_indices(n, n, offset=1)
    want = float(sub[iu[0], iu[1]].mean())
    assert abs(float(out.cpu()[0]) - want) <= U * want  # a float64 sum rounded once to float32


@pytest.mark.parametrize("t0,t", [(0, -1), (2, 11)])
def test_mmade_mmfde_equal_the_list_form_bitwise(t0, t, cuda):
    z, g = fixture_csr(cuda)
    futures = torch.from_numpy(z["futures"]).to(cuda)
    idx = [0, 3, 17, 42, 77, 99, 120, 149]
    gen = torch.Generator().manual_seed(19)
    pred = (futures[idx][:, None] + 0.5 * torch.randn(8, 5, 20, 16, 3, generator=gen).to(cuda)).contiguous()
    lists = g.mm_gt(futures, idx)
    assert [int(x.shape[0]) for x in lists] == np.diff(z["row_ptr"])[idx].tolist()
    for mine, listed in ((g.mmade, metrics.mmade), (g.mmfde, metrics.mmfde)):
        got = mine(pred, futures, idx, t0=t0, t=t)
        want = listed(futures[idx], pred, lists, t0=t0, t=t)
        assert got.shape == (8,) and torch.equal(bits(got), bits(want))
        assert torch.equal(bits(mine(pred, futures, torch.tensor(idx), t0=t0, t=t)), bits(want))


def _fed(acc, z, cuda, by_index=False, batches=BATCHES):
    pred = torch.from_numpy(z["apd_pred"]).to(cuda)
    for a, b in batches:
        acc.update(pred[a:b], segment_idx=torch.arange(a, b, device=cuda) if by_index else None)
    return acc


def test_apde_accumulator_on_the_device(cuda):
    z = golden("mmgt")
    table = torch.from_numpy(z["csv_gt_apd"]).to(cuda)
    want = float(z["apde"])
    acc = _fed(metrics.APDEAccumulator(table), z, cuda)
    assert acc.sum.device.type == "cuda" and acc.sum.dtype == torch.float64 and acc.count.dtype == torch.int64
    got = acc.compute()
    print(f"apde {got!r} vs reference {want!r}")
    assert abs(got - want) <= 1e-12 * want
    assert _fed(metrics.APDEAccumulator(table), z, cuda, by_index=True).compute() == got
    first, second = (_fed(metrics.APDEAccumulator(table), z, cuda, True, part) for part in (BATCHES[:1], BATCHES[1:]))
    merged = first.merge(second)
    assert abs(merged.compute() - got) <= 1e-12 * got and int(merged.count) == 145


def test_apde_from_the_device_table(cuda):
    """The whole chain: adjacency, GT-APD table, accumulator; against the reference storer fed the float64 table."""
    z = golden("mmgt")
    g = multimodal_gt.get_multimodal_gt(torch.from_numpy(z["obs"])[:, -1].to(cuda), float(z["thr"]))
    table = g.gt_apd(torch.from_numpy(z["futures"]).to(cuda))
    table[torch.from_numpy(z["csv_gt_apd"] == 0).to(cuda)] = 0  # the entries the fixture's CSV zeroes
    got = _fed(metrics.APDEAccumulator(table), z, cuda).compute()
    want = float(z["apde"])
    # every table entry is within 1e-5 relative of the float64 one (test_gt_apd_against_the_reference), and a
    # segment's error moves by at most its entry's: |got - want| <= 1e-5 * the largest entry
    assert abs(got - want) <= 1e-5 * float(z["gt_apd"].max()), (got, want)
