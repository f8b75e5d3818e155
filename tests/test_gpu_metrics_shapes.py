"""The first-generation metric kernels (sd_metrics.hip: k_pairwise, k_ade_fde, k_segment_mean behind
metrics.lat_apd / apd / ade / fde / mmade / mmfde and MultimodalGT.mmade / mmfde) against the float64 oracle at
ragged shapes: feature counts that are no multiple of the 64-feature chunk, frames wider than the 64 lanes, sample
counts around the pair-slot and wave-stride boundaries, more sequences than one block of k_segment_mean, NaN and
Inf.  The cases, the derivation of every bound and the exactness claims are in tests/metrics_cases.py;
tests/test_metrics.py proves the claims on the host.

Largest observed error as a fraction of its derived bound on the MI355X (the `[metrics-shapes]` lines of
profiles/metrics_shapes/pytest_gpu_metrics.txt).  Bounded tier: k_pairwise L1 0.029 and L2 0.024 (both at S = 3,
X = 63), k_ade_fde ade 0.200 (S = 64, T = 1, F = 63) and fde 0.222 (S = 64, T = 7, F = 64).  Exact tier: lat_apd,
ade, fde, mmade and mmfde equal the oracle to the bit in every case (error 0); apd 0.146 of its 4 ulp (S = 3,
X = 65: the one square root per pair).  With the parent's fminf minimum the three NaN cases fail (ade 3.88 where
the oracle says NaN; profiles/metrics_shapes/pytest_gpu_parent_library.txt) and every other test passes."""
import pytest
import torch

import metrics_cases as C
from skeletondiffusion_amd import _lib
from skeletondiffusion_amd import metrics as M
from skeletondiffusion_amd import multimodal_gt

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def held(what, got, ref, bound):
    """Print the figure, then hold `got` to `bound` relative to the float64 oracle's `ref`"""
    assert got.dtype == torch.float32
    err = C.rel_err(got, ref)
    print(f"\n[metrics-shapes] {what}: error {err:.3e}  bound {bound:.3e}  error / bound {err / bound:.3f}")
    assert err <= bound, (what, err, bound)


# ---- exact tier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,X", C.PAIR_SHAPES)
def test_pairwise_exact(S, X, cuda):
    c = C.pairwise_exact(S, X)
    x = c.x.to(cuda)
    held(f"exact lat_apd S={S} X={X}", M.lat_apd(x), c.lat_apd, C.PAIR_ULPS * C.ULP)
    held(f"exact apd S={S} X={X}", M.apd(x.unsqueeze(2)), c.apd, C.PAIR_ULPS * C.ULP)


def test_pairwise_position_sweep(cuda):
    c, _ = C.pairwise_sweep()
    x = c.x.to(cuda)
    held("sweep lat_apd", M.lat_apd(x), c.lat_apd, C.PAIR_ULPS * C.ULP)
    held("sweep apd", M.apd(x.unsqueeze(2)), c.apd, C.PAIR_ULPS * C.ULP)


def _ade_all(what, c, target, pred, ade_bound, fde_bound, **kw):
    held(f"{what} ade", M.ade(target, pred, **kw), c.ade, ade_bound)
    held(f"{what} fde", M.fde(target, pred, **kw), c.fde, fde_bound)
    held(f"{what} ade none", M.ade(target, pred, reduction="none", **kw), c.ade_none, ade_bound)
    held(f"{what} fde none", M.fde(target, pred, reduction="none", **kw), c.fde_none, fde_bound)


@pytest.mark.parametrize("S,T,F", C.ADE_SHAPES)
def test_ade_fde_exact(S, T, F, cuda):
    c = C.ade_exact(S, T, F)
    _ade_all(f"exact S={S} T={T} F={F}", c, c.target.to(cuda), c.pred.to(cuda), C.ADE_ULPS * C.ULP, C.ADE_ULPS * C.ULP)


def _per_sequence_bound(counts):
    return torch.tensor([C.mm_bound(n) for n in counts], dtype=torch.float64)


def _held_rows(what, got, ref, bounds):
    """as held(), each sequence against its own bound"""
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = (got.cpu().double() - ref.double()).abs() / ref.double()
    print(f"\n[metrics-shapes] {what}: largest error / bound {float((err / bounds).max()):.3f}")
    assert bool((err <= bounds).all()), (what, float((err / bounds).max()))


def test_mm_exact_two_blocks_and_a_long_segment(cuda):
    c = C.mm_exact()
    pred = c.pred.to(cuda)
    mm_gt = [g.to(cuda) for g in c.mm_gt]
    bounds = _per_sequence_bound(c.counts)
    _held_rows("exact mmade", M.mmade(None, pred, mm_gt), c.mmade, bounds)
    _held_rows("exact mmfde", M.mmfde(None, pred, mm_gt), c.mmfde, bounds)
    g = multimodal_gt.MultimodalGT(c.row_ptr, c.col, cuda)
    futures = c.futures.to(cuda)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(g.mm_gt(futures, c.segment_idx[-3:]), c.mm_gt[-3:]))
    _held_rows("exact MultimodalGT.mmade", g.mmade(pred, futures, c.segment_idx), c.mmade, bounds)
    _held_rows("exact MultimodalGT.mmfde", g.mmfde(pred, futures, c.segment_idx), c.mmfde, bounds)


# ---- bounded tier -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,X", C.PAIR_SHAPES)
def test_pairwise_bounded(S, X, cuda):
    c = C.pairwise_normal(S, X)
    x = c.x.to(cuda)
    held(f"k_pairwise L1 S={S} X={X}", M.lat_apd(x), c.lat_apd, C.pairwise_bound(X))
    held(f"k_pairwise L2 S={S} X={X}", M.apd(x.unsqueeze(2)), c.apd, C.pairwise_bound(X))


@pytest.mark.parametrize("S,T,F", C.ADE_SHAPES)
def test_ade_fde_bounded(S, T, F, cuda):
    c = C.ade_normal(S, T, F)
    _ade_all(f"k_ade_fde S={S} T={T} F={F}", c, c.target.to(cuda), c.pred.to(cuda), C.ade_bound(T, F), C.fde_bound(F))


def test_mano_rows_through_a_time_slice(cuda):
    """(2, 50, 8, 51, 3) with t0 = 2, t = 7: frames of F = 153, and the narrowed pred is not contiguous"""
    target, pred, apd, ade, fde = C.mano_case()
    target, pred = target.to(cuda), pred.to(cuda)
    T, F = C.MANO_T - C.MANO_T0, 153
    assert not pred.narrow(2, C.MANO_T0, T).is_contiguous()
    kw = dict(t0=C.MANO_T0, t=C.MANO_T)
    held("k_pairwise L2 mano slice", M.apd(pred, **kw), apd, C.pairwise_bound(T * F))
    held("k_ade_fde mano slice ade", M.ade(target, pred, **kw), ade, C.ade_bound(T, F))
    held("k_ade_fde mano slice fde", M.fde(target, pred, **kw), fde, C.fde_bound(F))


def test_permuted_view(cuda):
    stored, c, p = C.permuted_case()
    pred = stored.to(cuda).permute(0, 2, 1, 3)
    assert not pred.is_contiguous()
    S, T, F = C.PERM_S, C.PERM_T, C.PERM_F
    _ade_all("k_ade_fde permuted view", c, c.target.to(cuda), pred, C.ade_bound(T, F), C.fde_bound(F))
    held("k_pairwise L1 permuted view", M.lat_apd(pred), p.lat_apd, C.pairwise_bound(T * F))
    held("k_pairwise L2 permuted view", M.apd(pred), p.apd, C.pairwise_bound(T * F))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_other_input_types_are_cast_to_float32(dtype, cuda):
    target, pred, c, p = C.dtype_case(dtype)
    target, pred = target.to(cuda), pred.to(cuda)
    _, S, T, F = pred.shape
    _ade_all(f"k_ade_fde {dtype}", c, target, pred, C.ade_bound(T, F), C.fde_bound(F))
    held(f"k_pairwise L1 {dtype}", M.lat_apd(pred), p.lat_apd, C.pairwise_bound(T * F))
    held(f"k_pairwise L2 {dtype}", M.apd(pred), p.apd, C.pairwise_bound(T * F))


# ---- structure tier: bitwise ------------------------------------------------------------------------------------
def test_a_sequence_does_not_depend_on_its_batch(cuda):
    """One workgroup per sequence: the call on 5 sequences, five calls on one (read where it lies in the batch, on
    every 4-byte phase, and from a copy of its own) and the reversed batch give the same bits"""
    x, target, pred = (t.to(cuda) for t in C.structure_case())
    calls = {
        "lat_apd": (lambda i: M.lat_apd(x[i])),
        "apd": (lambda i: M.apd(x[i].unsqueeze(2))),
        "ade": (lambda i: M.ade(target[i], pred[i])),
        "fde": (lambda i: M.fde(target[i], pred[i])),
        "ade none": (lambda i: M.ade(target[i], pred[i], reduction="none")),
        "fde none": (lambda i: M.fde(target[i], pred[i], reduction="none")),
    }
    n = C.STRUCT_B
    assert sorted({(x[b:b + 1].data_ptr() // 4) % 4 for b in range(n)}) == [0, 1, 2, 3]
    assert sorted({(pred[b:b + 1].data_ptr() // 4) % 4 for b in range(n)}) == [0, 1, 2, 3]
    back = torch.arange(n - 1, -1, -1, device=cuda)
    for name, call in calls.items():
        whole = call(slice(None))
        assert whole.shape[0] == n
        singles = torch.cat([call(slice(b, b + 1)) for b in range(n)])
        assert same_bits(singles, whole), name
        assert same_bits(call(back), whole[back]), name


def test_identical_samples_and_a_perfect_sample_give_zero(cuda):
    x, target, pred = (t.to(cuda) for t in C.structure_case())
    same = x[:, :1].repeat(1, C.STRUCT_S, 1)
    zero = torch.zeros(C.STRUCT_B, device=cuda)
    assert same_bits(M.lat_apd(same), zero) and same_bits(M.apd(same.unsqueeze(2)), zero)
    for k in range(C.STRUCT_S):
        p = pred.clone()
        p[:, k] = target
        assert same_bits(M.ade(target, p), zero) and same_bits(M.fde(target, p), zero), k
        per = M.ade(target, p, reduction="none")
        assert not bool(per[:, k].any()) and bool((per[:, [s for s in range(C.STRUCT_S) if s != k]] > 0).all())


# ---- non-finite tier --------------------------------------------------------------------------------------------
def _raw_mm(pred, mm_gt):
    """sd_mm_ade_fde itself, all four outputs of one call: (pair_ade, pair_fde, mmade, mmfde)"""
    dev = pred.device
    Bn, S, T, F = pred.shape
    p = pred.contiguous()
    gts = torch.cat(mm_gt).contiguous()
    counts = torch.tensor([g.shape[0] for g in mm_gt])
    off = torch.zeros(Bn + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(counts, 0)
    seq = torch.repeat_interleave(torch.arange(Bn), counts).to(dev)
    off = off.to(dev)
    n = gts.shape[0]
    out = [torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(Bn, device=dev), torch.empty(Bn, device=dev)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib().sd_mm_ade_fde(p.data_ptr(), gts.data_ptr(), seq.data_ptr(), n, off.data_ptr(), Bn, S, T, F,
                                        *(o.data_ptr() for o in out), stream))
    torch.cuda.synchronize()
    return out, seq.cpu()


def _device_values(target, pred, mm_gt):
    (pair_ade, pair_fde, raw_mmade, raw_mmfde), seq = _raw_mm(pred, mm_gt)
    v = {"ade": M.ade(target, pred), "fde": M.fde(target, pred), "mmade": M.mmade(target, pred, mm_gt),
         "mmfde": M.mmfde(target, pred, mm_gt), "raw mmade": raw_mmade, "raw mmfde": raw_mmfde,
         "lat_apd": M.lat_apd(pred), "apd": M.apd(pred), "ade_none": M.ade(target, pred, reduction="none"),
         "fde_none": M.fde(target, pred, reduction="none"), "pair_ade": pair_ade, "pair_fde": pair_fde}
    return {k: t.cpu() for k, t in v.items()}, seq


@pytest.fixture(scope="module")
def nonfinite_clean(cuda):
    target, pred, mm_gt = C.nonfinite_clean()
    target, mm_gt = target.to(cuda), [g.to(cuda) for g in mm_gt]
    return target, mm_gt, _device_values(target, pred.to(cuda), mm_gt)[0]


def _oracle_name(name):
    return name.replace("raw ", "")


@pytest.mark.parametrize("k", C.NF_SAMPLES)
def test_a_nan_sample_makes_its_sequence_nan(k, nonfinite_clean, cuda):
    """One NaN element in sample k of sequence NF_SEQ: every value of that sequence is NaN exactly where torch.min /
    mean on the float64 CPU oracle give NaN, and every other value keeps the bits of the run without it"""
    target, mm_gt, clean = nonfinite_clean
    ref = C.nonfinite_case((k,), float("nan"))
    got, seq = _device_values(target, ref.pred.to(cuda), mm_gt)
    for name in ("ade", "fde", "mmade", "mmfde", "raw mmade", "raw mmfde", "lat_apd", "apd", "ade_none", "fde_none"):
        want_nan = torch.isnan(getattr(ref, _oracle_name(name)))
        assert int(want_nan.sum()) == 1
        assert torch.equal(torch.isnan(got[name]), want_nan), (name, got[name])
        assert torch.equal(bits(got[name][~want_nan]), bits(clean[name][~want_nan])), name
    assert bool(torch.isnan(got["ade_none"][C.NF_SEQ, k])) and bool(torch.isnan(got["fde_none"][C.NF_SEQ, k]))
    for name in ("pair_ade", "pair_fde"):  # every pair of the sequence, and no other
        assert torch.equal(torch.isnan(got[name]), seq == C.NF_SEQ), (name, got[name])
        assert torch.equal(bits(got[name][seq != C.NF_SEQ]), bits(clean[name][seq != C.NF_SEQ])), name


@pytest.mark.parametrize("samples", [(k,) for k in C.NF_SAMPLES] + [tuple(range(C.NF_S))], ids=str)
def test_inf_samples_lose_the_minimum(samples, nonfinite_clean, cuda):
    """+Inf in one sample: its distance is +Inf and the minimum passes it over; in every sample: the minimum is +Inf"""
    target, mm_gt, clean = nonfinite_clean
    ref = C.nonfinite_case(samples, float("inf"))
    got, seq = _device_values(target, ref.pred.to(cuda), mm_gt)
    T, F = C.NF_T, C.NF_F
    for name in ("ade", "fde", "mmade", "mmfde", "raw mmade", "raw mmfde", "ade_none", "fde_none"):
        want = getattr(ref, _oracle_name(name))
        inf = torch.isinf(want)
        assert torch.equal(got[name] == float("inf"), inf), (name, got[name])
        assert int(inf.sum()) == (len(samples) if "none" in name else int(len(samples) == C.NF_S)), name
        bound = C.fde_bound(F) if "fde" in name else C.ade_bound(T, F)
        held(f"inf {samples} {name}", got[name][~inf], want[~inf], bound + (max(C.NF_COUNTS) + 2) * C.U * ("mm" in name))
        others = torch.arange(C.B) != C.NF_SEQ
        assert torch.equal(bits(got[name][others]), bits(clean[name][others])), name
