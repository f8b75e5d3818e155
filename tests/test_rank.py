"""Host side of the diversity ranking, the class-wise CMD and the metric storers: the C ABI
and its argument checks, the CPU refusals of the ranking wrappers, the accumulators on CPU tensors against
the fixture of the reference's own storers, and the fixture's picks re-derived by a float64 greedy written
here.  No GPU; the device tests are in tests/test_gpu_rank.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rank_cases as R
from conftest import REPO
from skeletondiffusion_amd import _lib, evaluation, metrics
from skeletondiffusion_amd._lib import SkelDiffError

ENTRIES = ("sd_diverse_rank_workspace_bytes", "sd_diverse_rank", "sd_class_sum")


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bsize_t sd_diverse_rank_workspace_bytes\(int64_t nseq, int32_t samples\)", hdr)
    assert re.search(r"\bint sd_diverse_rank\(const float\* pred, const float\* target, int64_t nseq, int32_t samples, "
                     r"int64_t features,\s+int32_t n_choose, int32_t from_closest, int64_t\* idx_out, float\* score_out, "
                     r"int64_t\* closest_out,\s+float\* dist_out, void\* workspace, size_t workspace_bytes, void\* stream\)", hdr)
    assert re.search(r"\bint sd_class_sum\(const float\* values, const int64_t\* cls, int64_t rows, int32_t width, "
                     r"int32_t classes, double\* sum,\s+int64_t\* count, int64_t\* total, void\* stream\)", hdr)
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    for lines in ("ranking.py:3-40", ":42-63", "cmd.py:15-31", ":34-57", "No index found"):  # the reference lines replaced
        assert lines in hdr, lines
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4


def test_host_argument_checks():
    """Every argument is refused by name on the host, before any launch."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)
    big = 1 << 40

    def rank(pred=p, target=p, nseq=2, samples=5, features=7, n=3, fc=0, idx=p, score=None, closest=None, dist=None, ws=p,
             ws_bytes=big):
        return L.sd_diverse_rank(pred, target, nseq, samples, features, n, fc, idx, score, closest, dist, ws, ws_bytes, None)

    def csum(values=p, cls=p, rows=3, width=4, classes=2, s=p, count=p, total=p):
        return L.sd_class_sum(values, cls, rows, width, classes, s, count, total, None)

    assert L.sd_diverse_rank_workspace_bytes(2, 5) == 2 * 6 * 6 * 4
    assert L.sd_diverse_rank_workspace_bytes(256, 255) == 256 * 256 * 256 * 4
    for bad in ((-1, 5), (2, 0), (2, 256)):
        assert L.sd_diverse_rank_workspace_bytes(*bad) == 0
    for call, cases in (
            (rank, ((dict(pred=None), b"pred is null"), (dict(target=None), b"target is null"), (dict(idx=None), b"idx_out is null"),
                    (dict(ws=None), b"workspace is null"), (dict(ws_bytes=2 * 6 * 6 * 4 - 1), b"workspace_bytes"),
                    (dict(nseq=-1), b"nseq"), (dict(samples=0), b"samples"), (dict(samples=-3), b"samples"),
                    (dict(samples=256, n=3), b"samples must be in 1..255"), (dict(features=0), b"features"),
                    (dict(features=-2), b"features"), (dict(n=0), b"n_choose"), (dict(n=6), b"n_choose"),
                    (dict(n=-1), b"n_choose"), (dict(fc=2), b"from_closest"), (dict(fc=-1), b"from_closest"),
                    (dict(closest=p), b"closest_out"), (dict(nseq=1 << 31, samples=255, n=3), b"tile pairs"))),
            (csum, ((dict(values=None), b"values is null"), (dict(cls=None), b"cls is null"), (dict(s=None), b"sum is null"),
                    (dict(count=None), b"count is null"), (dict(total=None), b"total is null"), (dict(rows=-1), b"rows"),
                    (dict(width=0), b"width"), (dict(width=-4), b"width"), (dict(classes=0), b"classes")))):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())
    # no sequences / rows: a successful no-op (nothing is launched: the pointers above are host addresses)
    assert rank(nseq=0, pred=None, target=None, idx=None, ws=None, ws_bytes=0) == 0
    assert csum(rows=0, values=None, cls=None, s=None, count=None, total=None) == 0


def test_cpu_tensors_are_refused_by_name():
    z = R.fixture()
    pred, tgt = torch.from_numpy(z["rank0_pred"]), torch.from_numpy(z["rank0_target"])
    for call in (lambda: metrics.diverse_rank(pred, tgt, 3), lambda: metrics.diverse_rank(pred, tgt, 3, from_closest=True),
                 lambda: metrics.find_samples_maxapd_wrtGT(pred, tgt, 3),
                 lambda: metrics.get_closest_and_nfurthest_maxapd(pred[0], tgt[0], 2),
                 lambda: metrics.get_closest_and_nfurthest_maxapd(pred, tgt, 2)):
        with pytest.raises(SkelDiffError, match="HIP engine only"):
            call()
    with pytest.raises(ValueError, match="diverse_rank"):
        metrics.diverse_rank(pred, tgt[:, :2], 3)
    with pytest.raises(AssertionError):
        metrics.get_closest_and_nfurthest_maxapd(pred[0, :, :, :, :2], tgt[0], 2)
    factory, transform = evaluation.get_cmd_storer(["a", "b"], [0.1, 0.2], device="cpu")
    assert isinstance(factory(output_transform=None), metrics.CMDAccumulator)
    with pytest.raises(SkelDiffError, match="HIP engine only"):  # motion_for_cmd is a kernel
        transform(pred=pred, class_idx=[0, 1, 0])
    with pytest.raises(ValueError):
        evaluation.get_cmd_storer(["a", "b"], [0.1])


def test_fixture_picks_are_the_float64_greedy():
    """The reference's lists equal the specification's greedy on float64 distances, with a clear margin
    at every pick (the generator's condition, re-derived)."""
    z = R.fixture()
    for c in range(R.RANK_CASES):
        pred, tgt, idx = z[f"rank{c}_pred"], z[f"rank{c}_target"], z[f"rank{c}_idx"]
        assert pred.dtype == np.float32 and idx.dtype == np.int64 and idx.shape[0] == pred.shape[0]
        for b in range(pred.shape[0]):
            picks, _ = R.greedy(R.dist64(np.concatenate([tgt[b][None], pred[b]])), idx.shape[1])
            assert picks.tolist() == idx[b].tolist(), (c, b)
    pred, gt, idx, first = z["closest_pred"], z["closest_gt"], z["closest_idx"], int(z["closest_first"])
    d = R.dist64(np.concatenate([gt[None], pred]))
    assert R.closest(d) == first
    picks, scores = R.greedy(d, len(idx), anchor=1 + first)
    assert picks.tolist() == idx.tolist() and first not in idx.tolist()
    # the twin of the anchor is at distance exactly 0: the last of a full ranking
    full, scores = R.greedy(d, pred.shape[0], anchor=1 + first)
    assert full[-1] == first and scores[-1] == 0.0 and sorted(full.tolist()) == list(range(pred.shape[0]))


def test_greedy_restatement_orders_ties_and_nan():
    d = np.array([[0, 2, 2, 1], [2, 0, 0, 1], [2, 0, 0, 1], [1, 1, 1, 0]], dtype=np.float32)
    assert R.greedy(d, 3)[0].tolist() == [0, 2, 1]  # 1 and 2 tie at 2: the lower; then 3 (1) before the twin (0)
    d[2, :] = d[:, 2] = np.nan
    picks, scores = R.greedy(d, 3)
    assert picks.tolist() == [0, 2, 1] and np.isnan(scores[2])  # the NaN sample last
    assert R.closest(np.array([[0, np.nan, 3, 3]], dtype=np.float32)) == 1


def test_cmd_accumulator_on_cpu_tensors():
    z = R.fixture()
    motion, cls, ref = torch.from_numpy(z["cmd_motion"]), z["cmd_cls"], z["cmd_ref"]
    value, per_class, bound = R.cmd_float64(z["cmd_motion"], cls, ref)
    whole = metrics.CMDAccumulator(ref)
    whole.update(motion, cls)
    assert whole.sum.dtype == torch.float64 and whole.count.tolist() == [4, 4, 0, 3] and int(whole.total) == 12
    assert whole.compute() == pytest.approx(value, rel=1e-12)
    assert abs(whole.compute() - float(z["cmd_value"])) <= bound
    mpc = whole.motion_per_class()
    assert mpc.dtype == torch.float64 and torch.equal(mpc[2], torch.zeros(9, dtype=torch.float64))
    np.testing.assert_allclose(mpc.numpy(), per_class, rtol=1e-12)
    parts = metrics.CMDAccumulator(ref)
    for a in range(0, 12, 4):
        parts.update(motion[a:a + 4], torch.from_numpy(cls[a:a + 4]))
    assert torch.equal(parts.sum, whole.sum) and torch.equal(parts.count, whole.count) and torch.equal(parts.total, whole.total)
    halves = [metrics.CMDAccumulator(ref), metrics.CMDAccumulator(ref)]
    halves[0].update(motion[:6], cls[:6])
    halves[1].update(motion[6:], list(cls[6:]))
    assert halves[0].merge(halves[1]).compute() == pytest.approx(value, rel=1e-12)
    whole.reset()
    with pytest.raises(SkelDiffError, match="at least one update"):
        whole.compute()
    with pytest.raises(ValueError):
        parts.update(motion[:, :5], cls)
    with pytest.raises(ValueError):
        parts.update(motion, cls[:3])


def test_metric_accumulator_on_cpu_tensors():
    z = R.fixture()
    values = torch.from_numpy(z["storer_values"])
    exact = {"mean": float(values.double().sum() / len(values)), "max": float(values.max()), "min": float(values.min())}
    exact["avg"] = exact["mean"]
    for op in ("mean", "avg", "max", "min"):
        acc = metrics.MetricAccumulator(op)
        for a in range(0, len(values), R.STORER_BATCH):
            acc.update(values[a:a + R.STORER_BATCH])
        assert acc.cumulator.dtype == torch.float64
        assert acc.compute() == pytest.approx(exact[op], rel=1e-12), op
        assert acc.compute() == pytest.approx(float(z[f"storer_{op}"]), rel=1e-5), op
        two = [metrics.MetricAccumulator(op), metrics.MetricAccumulator(op)]
        two[0].update(values[:50])
        two[1].update(values[50:])
        assert two[0].merge(two[1]).compute() == pytest.approx(exact[op], rel=1e-12), op
    # the reference's starting values (metric_storer.py:16): a maximum of negatives is 0, a minimum above 1e6 is 1e6
    acc = metrics.MetricAccumulator("max")
    acc.update(torch.from_numpy(z["storer_neg"]))
    assert acc.compute() == float(z["storer_max_neg"]) == 0.0
    acc = metrics.MetricAccumulator("min")
    acc.update(torch.from_numpy(z["storer_big"]))
    assert acc.compute() == float(z["storer_min_big"]) == 1000000.0
    # (B, k) values: one result per column
    acc = metrics.MetricAccumulator("avg")
    acc.update(values[:128].reshape(64, 2))
    np.testing.assert_allclose(acc.compute().numpy(), values[:128].double().reshape(64, 2).mean(0).numpy(), rtol=1e-12)
    with pytest.raises(AssertionError):
        metrics.MetricAccumulator("median")
    with pytest.raises(SkelDiffError, match="at least one example"):
        metrics.MetricAccumulator("avg").compute()


def test_metric_set_storers_match_the_flags():
    """config_metrics.py:71-96: which storers exist; built on the CPU (no kernel runs before update)."""
    gt_apd = torch.ones(4, dtype=torch.float64)
    cmd_kw = dict(idx_to_class=["a", "b"], mean_motion_per_class=[0.1, 0.2])
    base = set(evaluation.get_stats_funcs("probabilistic", "h36m16"))
    ms = evaluation.metric_set("probabilistic", "h36m16", device="cpu")
    assert set(ms.storers) == base and all(isinstance(s, metrics.MetricAccumulator) for s in ms.storers.values())
    assert all(s.return_op == "avg" for s in ms.storers.values())
    ms = evaluation.metric_set("probabilistic", "h36m16", if_compute_cmd=True, if_compute_apde=True, gt_apd=gt_apd, device="cpu",
                               **cmd_kw)
    assert set(ms.storers) == base | {"CMD", "APDE"}
    assert isinstance(ms.storers["CMD"], metrics.CMDAccumulator) and isinstance(ms.storers["APDE"], metrics.APDEAccumulator)
    ms = evaluation.metric_set("probabilistic", "h36m16", dataset_split="valid", if_compute_cmd=True, if_compute_fid=True,
                               device="cpu", **cmd_kw)
    assert set(ms.storers) == base  # CMD and FID belong to the test split
    ms = evaluation.metric_set("deterministic", "amass21", dataset_name="amass", if_compute_fid=True, device="cpu")
    assert set(ms.storers) == set(evaluation.get_stats_funcs("deterministic", "amass21"))  # FID is h36m's
    with pytest.raises(NotImplementedError):
        evaluation.metric_set("other", "h36m16")
