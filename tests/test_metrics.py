"""On-device evaluation metrics (skeletondiffusion_amd.metrics) against the reference's own
src/metrics/multimodal.py outputs (tests/golden/metrics.npz, made by gen_golden.py) and the
oracle's restatement.  Tolerance: relative 1e-5 (fp32 sums over up to 1536 features, fixed order
on the device, cdist / float64 on the host)."""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import golden
from skeletondiffusion_amd import synthetic

RTOL = 1e-5


def _inputs():
    lat = torch.from_numpy(synthetic.normal((3, 50, 16, 96), seed=31)) * 0.3
    motion = torch.from_numpy(synthetic.normal((2, 7, 20, 16, 3), seed=32))
    target = torch.from_numpy(synthetic.normal((2, 20, 16, 3), seed=33))
    return lat, motion, target


def _close(a, b):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + 1e-6), (a, b)


def test_oracle_metrics_match_reference():
    z = golden("metrics")
    lat, motion, target = _inputs()
    _close(O.metric_lat_apd(lat), z["lat_apd"])
    _close(O.metric_apd(lat.unsqueeze(2)), z["lat_apd_l2"])
    _close(O.metric_apd(motion), z["apd"])
    _close(O.metric_apd(motion, 5, 15), z["apd_t5_15"])
    _close(O.metric_ade(target, motion), z["ade"])
    _close(O.metric_ade(target, motion, 5, 15), z["ade_t5_15"])
    _close(O.metric_ade(target, motion, last_only=True), z["fde"])
    _close(O.metric_ade(target, motion, reduction="none"), z["ade_per_sample"])
    _close(O.metric_ade(target, motion, reduction="none", last_only=True), z["fde_per_sample"])


def test_metrics_refuse_cpu_tensors():
    from skeletondiffusion_amd import metrics
    from skeletondiffusion_amd._lib import SkelDiffError

    with pytest.raises(SkelDiffError):
        metrics.lat_apd(torch.zeros(2, 3, 4))


@pytest.mark.gpu
def test_device_metrics_match_reference(cuda):
    from skeletondiffusion_amd import metrics as M

    z = golden("metrics")
    lat, motion, target = (t.to(cuda) for t in _inputs())
    _close(M.lat_apd(lat), z["lat_apd"])
    _close(M.apd(lat.unsqueeze(2)), z["lat_apd_l2"])
    _close(M.apd(motion), z["apd"])
    _close(M.apd(motion, t0=5, t=15), z["apd_t5_15"])
    _close(M.ade(target, motion), z["ade"])
    _close(M.ade(target, motion, t0=5, t=15), z["ade_t5_15"])
    _close(M.fde(target, motion), z["fde"])
    _close(M.ade(target, motion, reduction="none"), z["ade_per_sample"])
    _close(M.fde(target, motion, reduction="none"), z["fde_per_sample"])


@pytest.mark.gpu
def test_device_metrics_deterministic_and_edges(cuda):
    from skeletondiffusion_amd import metrics as M
    from skeletondiffusion_amd._lib import SkelDiffError

    g = torch.Generator(device=cuda).manual_seed(5)
    lat = torch.randn(4, 64, 16, 96, device=cuda, generator=g)   # 64 samples: the maximum
    a, b = M.lat_apd(lat), M.lat_apd(lat)
    assert torch.equal(a, b)
    _close(a, O.metric_lat_apd(lat.cpu()).numpy())
    one = torch.randn(3, 1, 5, 7, device=cuda, generator=g)
    assert torch.equal(M.apd(one).cpu(), torch.zeros(3, dtype=torch.int64))   # multimodal.py:19-20
    _close(M.ade(one[:, 0], one), np.zeros(3))
    with pytest.raises(SkelDiffError):
        M.lat_apd(torch.randn(2, 65, 8, device=cuda))
    empty = torch.zeros(0, 50, 16, 96, device=cuda)
    assert M.lat_apd(empty).shape == (0,)


@pytest.mark.gpu
def test_lat_apd_of_sampled_futures(cuda):
    """The metric on the sampler's own output: 2 sequences x 50 futures of the release Denoiser."""
    from conftest import build_release_diffusion, release_inputs
    from skeletondiffusion_amd import metrics as M

    z = golden("release_h36m16_T10")
    d = build_release_diffusion(z, cuda)
    xcs = torch.from_numpy(synthetic.uniform((2, 16, 96), 41)).to(cuda)
    img, _ = d.sample(batch_size=100, x_cond=xcs)
    lat = img.view(2, 50, 16, 96)
    _close(M.lat_apd(lat), O.metric_lat_apd(lat.cpu()).numpy())
    _close(M.apd(lat.unsqueeze(2)), O.metric_apd(lat.unsqueeze(2).cpu()).numpy())


# ---- the design claims of tests/metrics_cases.py (the cases of tests/test_gpu_metrics_shapes.py), without a device --

def _same(oracle_f32, by_hand_f64):
    """the oracle's float32 result is the float64 hand value, cast"""
    assert oracle_f32.dtype == torch.float32
    assert torch.equal(oracle_f32, by_hand_f64.float()), (oracle_f32, by_hand_f64)


def test_exact_pairwise_cases_are_integer_sums_below_2_24():
    import metrics_cases as C

    assert {S for S, _ in C.PAIR_SHAPES} == set(C.PAIR_S) and {X for _, X in C.PAIR_SHAPES} == set(C.PAIR_X)
    for S, X in C.PAIR_SHAPES:
        c = C.pairwise_exact(S, X)
        assert c.x.shape == (C.B, S, X) and torch.equal(c.x, c.x.round()) and float(c.x.abs().max()) <= 8
        l1, l2sq = C.pair_sums(c.x)
        assert l1.shape == (C.B, S * (S - 1) // 2)
        assert int(l1.max()) < C.LIMIT and int(l2sq.max()) < C.LIMIT and int(l2sq.max()) <= 256 * X
        _same(c.lat_apd, l1.double().mean(-1))  # an exact float64 sum of integers, one division
        # the roots are irrational or exact; their float64 mean may round otherwise than the oracle's by an ulp of float64
        assert C.rel_err(c.apd, l2sq.double().sqrt().mean(-1)) <= C.U
    c, want = C.pairwise_sweep()
    assert c.x.shape == (len(C.SWEEP_POSITIONS), C.SWEEP_S, C.SWEEP_X) and len(set(C.SWEEP_COEFFS)) == C.SWEEP_S
    assert max(C.SWEEP_POSITIONS) == C.SWEEP_X - 1 and float(c.x.abs().max()) < 32
    l1, l2sq = C.pair_sums(c.x)
    assert int(l2sq.max()) < C.LIMIT
    for q, f in enumerate(C.SWEEP_POSITIONS):  # the samples of sequence q differ at position f alone
        differ = (c.x[q] != c.x[q, :1]).any(0).nonzero().flatten().tolist()
        assert differ == [f]
    assert torch.equal(l1 * l1, l2sq)  # one differing feature: L2 = L1 = |c_i - c_j|
    _same(c.lat_apd, want)
    _same(c.apd, want)


def test_exact_ade_cases_are_known_integers():
    import metrics_cases as C

    shapes = C.ADE_SHAPES
    assert 24 <= len(shapes) <= 48 and len(set(shapes)) == len(shapes) and set(C.ADE_KEEP) <= set(shapes)
    for axis, values in enumerate((C.ADE_S, C.ADE_T, C.ADE_F)):
        assert {s[axis] for s in shapes} == set(values)
    hit = {F: set() for F in C.ADE_F}
    last_min = {"ade": False, "fde": False}
    for S, T, F in shapes:
        c = C.ade_exact(S, T, F)
        assert c.pred.shape == (C.B, S, T, F) and torch.equal(c.pred, c.pred.round()) and torch.equal(c.target, c.target.round())
        assert int(c.m.min()) >= 1 and int(c.m.max()) <= 7 and float(c.pred.abs().max()) <= 15
        # pred - target is m at feature f of each frame and 0 elsewhere
        diff = (c.pred - c.target[:, None]).to(torch.int64)
        want = torch.zeros_like(diff).scatter_(3, c.f[..., None], c.m[..., None])
        assert torch.equal(diff, want)
        assert int((c.m * c.m).max()) < C.LIMIT and int(c.m.sum(-1).max()) < C.LIMIT
        marks = C.ade_marks(F)
        assert marks[-1] == F - 1 and set(c.f.flatten().tolist()) <= set(marks)
        if C.B * S * T >= len(marks):
            assert set(c.f.flatten().tolist()) == set(marks)
        assert int(c.f[-1, -1, -1]) == F - 1  # the last frame of the last sample: the buffer's last element
        hit[F] |= set(c.f.flatten().tolist())
        per, last, ade, fde = C.ade_by_hand(c.m)
        _same(c.ade_none, per)
        _same(c.fde_none, last)
        _same(c.ade, ade)
        _same(c.fde, fde)
        if S > 1 and T > 1:  # the two minima are at different samples, each unique
            ia, il = per.argmin(-1), last.argmin(-1)
            assert bool((ia != il).all())
            assert bool(((per == ade[:, None]).sum(-1) == 1).all()) and bool(((last == fde[:, None]).sum(-1) == 1).all())
            last_min["ade"] |= bool((ia == S - 1).any())
            last_min["fde"] |= bool((il == S - 1).any())
    assert all(hit[F] == set(C.ade_marks(F)) for F in C.ADE_F) and all(last_min.values())


def test_exact_mm_case_is_known_integers():
    import metrics_cases as C

    c = C.mm_exact()
    assert c.pred.shape == (C.MM_SEQ, C.MM_S, C.MM_T, C.MM_F) and C.MM_SEQ > 256
    assert c.counts[C.MM_LONG[0]] == C.MM_LONG[1] and C.MM_LONG[0] >= 256
    assert set(c.counts) == set(C.MM_COUNTS) | {C.MM_LONG[1]}
    assert [int(g.shape[0]) for g in c.mm_gt] == c.counts
    for q in (0, 1, 2, C.MM_LONG[0], C.MM_SEQ - 1):  # the frame distances are m + n
        d = (c.pred[q][None] - c.mm_gt[q][:, None]).pow(2).sum(-1).sqrt()  # (count, S, T)
        assert torch.equal(d.to(torch.int64), c.m[q][None] + c.n[q][:, None]) and torch.equal(d, d.round())
    mmade, mmfde = C.mm_by_hand(c.m, c.n)
    _same(c.mmade, mmade)
    _same(c.mmfde, mmfde)
    # the CSR form of the same sets
    assert c.futures.shape == (sum(c.counts), C.MM_T, C.MM_F) and len(c.row_ptr) == sum(c.counts) + 1
    for q in (0, 2, C.MM_LONG[0], C.MM_SEQ - 1):
        a, b = int(c.row_ptr[c.segment_idx[q]]), int(c.row_ptr[c.segment_idx[q] + 1])
        assert torch.equal(c.futures[c.col[a:b]], c.mm_gt[q])


def test_oracle_propagates_nan_and_passes_over_inf():
    import metrics_cases as C

    target, clean_pred, mm_gt = C.nonfinite_clean()
    clean = C.nonfinite_case((), 0.0)
    assert torch.equal(clean.pred, clean_pred) and bool(torch.isfinite(clean.ade_none).all())
    b, others = C.NF_SEQ, [q for q in range(C.B) if q != C.NF_SEQ]
    assert C.NF_SAMPLES == (0, C.NF_S // 2, C.NF_S - 1)
    for k in C.NF_SAMPLES:
        c = C.nonfinite_case((k,), float("nan"))
        assert int(torch.isnan(c.pred).sum()) == 1
        for name in ("ade", "fde", "mmade", "mmfde", "lat_apd", "apd"):
            v, v0 = getattr(c, name), getattr(clean, name)
            assert bool(torch.isnan(v[b])) and torch.equal(v[others], v0[others]), name
        for name in ("ade_none", "fde_none"):
            v, v0 = getattr(c, name), getattr(clean, name)
            nan = torch.isnan(v)
            assert bool(nan[b, k]) and int(nan.sum()) == 1 and torch.equal(v[~nan], v0[~nan]), name
        # one +Inf sample: its own distance is +Inf, the minimum is that of the other samples
        c = C.nonfinite_case((k,), float("inf"))
        for name in ("ade", "fde"):
            per, per0 = getattr(c, name + "_none"), getattr(clean, name + "_none")
            assert float(per[b, k]) == float("inf") and int(torch.isinf(per).sum()) == 1
            rest = [s for s in range(C.NF_S) if s != k]
            assert float(getattr(c, name)[b]) == float(per0[b, rest].min())
        assert bool(torch.isfinite(c.mmade).all()) and bool(torch.isfinite(c.mmfde).all())
    c = C.nonfinite_case(tuple(range(C.NF_S)), float("inf"))
    for name in ("ade", "fde", "mmade", "mmfde"):
        v = getattr(c, name)
        assert float(v[b]) == float("inf") and torch.equal(v[others], getattr(clean, name)[others]), name


def test_bounded_tier_is_never_looser_than_rtol():
    import metrics_cases as C

    shapes = C.bounded_shapes()
    assert {k for k, _, _ in shapes} == {"pairwise", "ade", "fde"} and len(shapes) > 2 * len(C.ADE_SHAPES)
    for kernel, shape, bound in shapes:
        assert 8 * C.U <= bound < RTOL, (kernel, shape, bound)
    assert max(C.mm_bound(c) for c in C.mm_counts()) < RTOL
    assert C.PAIR_ULPS * C.ULP < RTOL and C.ADE_ULPS * C.ULP < RTOL
    # the cases the bounded tier adds build, and their references are finite
    _, _, apd, ade, fde = C.mano_case()
    assert apd.shape == ade.shape == fde.shape == (C.MANO_SHAPE[0],)
    stored, c, p = C.permuted_case()
    assert torch.equal(stored.permute(0, 2, 1, 3), c.pred) and bool(torch.isfinite(p.apd).all())
    for dt in C.DTYPES:
        target, pred, c, p = C.dtype_case(dt)
        assert target.dtype == pred.dtype == dt and bool(torch.isfinite(c.ade).all()) and bool(torch.isfinite(p.lat_apd).all())


def _mm_inputs():
    """tests/golden/gen_golden.py:mm_inputs (3 sequences, 3 / 1 / 2 multimodal ground truths)."""
    motion = torch.from_numpy(synthetic.normal((3, 7, 20, 16, 3), seed=34))
    gts = torch.from_numpy(synthetic.normal((4, 20, 16, 3), seed=35))
    target = torch.from_numpy(synthetic.normal((3, 20, 16, 3), seed=36))
    return motion, [gts[:3], gts[3:4], gts[1:3]], target


def test_oracle_mm_metrics_match_reference():
    z = golden("metrics")
    motion, mm_gt, _ = _mm_inputs()
    _close(O.metric_mmade(motion, mm_gt), z["mmade"])
    _close(O.metric_mmade(motion, mm_gt, last_only=True), z["mmfde"])
    _close(O.metric_mmade(motion, mm_gt, 5, 15), z["mmade_t5_15"])
    assert bool(z["mm_empty_raises"])  # the reference raises for a sequence without ground truths


@pytest.mark.gpu
def test_device_mm_metrics_match_reference(cuda):
    from skeletondiffusion_amd import _lib
    from skeletondiffusion_amd import metrics as M

    z = golden("metrics")
    motion, mm_gt, target = _mm_inputs()
    motion, target = motion.to(cuda), target.to(cuda)
    mm_gt = [g.to(cuda) for g in mm_gt]
    _close(M.mmade(target, motion, mm_gt), z["mmade"])
    _close(M.mmfde(target, motion, mm_gt), z["mmfde"])
    _close(M.mmade(target, motion, mm_gt, t0=5, t=15), z["mmade_t5_15"])
    with pytest.raises(RuntimeError):
        M.mmade(target, motion, [mm_gt[0], mm_gt[1], mm_gt[2][:0]])
    # the C ABI itself: a sequence without ground truths -> NaN; nseq == 0 is a no-op
    p = motion.reshape(3, 7, 20, 48).contiguous()
    g = torch.cat([mm_gt[0], mm_gt[1]]).reshape(4, 20, 48).contiguous()
    off = torch.tensor([0, 3, 4, 4], dtype=torch.int64, device=cuda)
    seq = torch.tensor([0, 0, 0, 1], dtype=torch.int64, device=cuda)
    pa, out = torch.empty(4, device=cuda), torch.empty(3, device=cuda)
    L = _lib.lib()
    assert L.sd_mm_ade_fde(p.data_ptr(), g.data_ptr(), seq.data_ptr(), 4, off.data_ptr(), 3, 7, 20, 48,
                           pa.data_ptr(), None, out.data_ptr(), None, 0) == 0
    torch.cuda.synchronize()
    _close(out[:2], z["mmade"][:2])
    assert torch.isnan(out[2])
    assert L.sd_mm_ade_fde(None, None, None, 0, None, 0, 7, 20, 48, None, None, None, None, 0) == 0
