"""Diversity ranking, class-wise CMD and the metric storers on the device.
  * the fixture of the reference's own ranking.py / cmd.py / metric_storer.py (tests/golden/rank.npz);
  * the bitwise contract of sd_diverse_rank: dist_out is sd_cdist of each sequence's [anchor; pred], idx and
    score are the greedy of rank_cases.greedy on that float32 matrix, at samples + 1 in {2, 64, 65, 130},
    features in {1, 9, 36, 4800}, n_choose in {1, samples}, 1 and 37 sequences, and a pred 4 bytes off a
    16-byte boundary;
  * ties, duplicates and NaN;
  * CMDAccumulator / MetricAccumulator against float64 and the reference within the bounds of the reference's
    float32 sums; metric_set against the metric functions' own batch means."""
import numpy as np
import pytest
import torch

import rank_cases as R
from skeletondiffusion_amd import evaluation, metrics, multimodal_gt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return R.fixture()


# ---- the reference's fixture -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(R.RANK_CASES))
def test_find_samples_maxapd_matches_the_reference(z, cuda, case):
    pred, tgt = torch.from_numpy(z[f"rank{case}_pred"]).to(cuda), torch.from_numpy(z[f"rank{case}_target"]).to(cuda)
    ref = z[f"rank{case}_idx"]
    none, idx = metrics.find_samples_maxapd_wrtGT(pred, tgt, num_chosen_samples=ref.shape[1])
    assert none is None and idx.dtype == torch.int64 and idx.device.type == "cuda"
    assert idx.tolist() == ref.tolist()  # the reference's list of lists
    r = metrics.diverse_rank(pred, tgt, ref.shape[1])
    assert r.closest is None and torch.equal(r.idx, idx) and r.score.shape == idx.shape
    assert bool((r.score[:, 1:] <= r.score[:, :-1]).all())  # a greedy's scores never grow


def test_closest_and_nfurthest_matches_the_reference(z, cuda):
    pred, gt = torch.from_numpy(z["closest_pred"]).to(cuda), torch.from_numpy(z["closest_gt"]).to(cuda)
    ref, first = z["closest_idx"], int(z["closest_first"])
    pc, sp, idx = metrics.get_closest_and_nfurthest_maxapd(pred, gt, len(ref))
    assert idx.tolist() == ref.tolist()
    assert torch.equal(pc, pred[first]) and torch.equal(sp, pred[torch.from_numpy(ref).to(cuda)])
    r = metrics.diverse_rank(pred[None], gt[None], len(ref), from_closest=True)
    assert r.closest.tolist() == [first] and r.idx.tolist() == [ref.tolist()]
    # a leading batch axis: the same answers per sequence
    pb, gb = torch.stack([pred, pred.flip(0)]), torch.stack([gt, gt])
    pcb, spb, idxb = metrics.get_closest_and_nfurthest_maxapd(pb, gb, len(ref))
    S = pred.shape[0]
    assert idxb[0].tolist() == ref.tolist() and idxb[1].tolist() == [S - 1 - i for i in ref.tolist()]
    assert torch.equal(pcb[0], pc) and torch.equal(pcb[1], pc) and torch.equal(spb[0], sp) and torch.equal(spb[1], sp)


# ---- the bitwise contract ----------------------------------------------------------------------------------------
def _expected(pred, tgt, from_closest):
    """per sequence: sd_cdist of [target; pred], the closest sample, sd_cdist of [anchor; pred]"""
    B, S = pred.shape[:2]
    dists, firsts = [], []
    for b in range(B):
        pts = torch.cat([tgt[b].reshape(1, -1), pred[b].reshape(S, -1)])
        d = multimodal_gt.cdist(pts, pts)
        c = None
        if from_closest:
            c = R.closest(d.cpu().numpy())
            pts = torch.cat([pred[b, c].reshape(1, -1), pred[b].reshape(S, -1)])
            d = multimodal_gt.cdist(pts, pts)
        dists.append(d)
        firsts.append(c)
    return torch.stack(dists), firsts


def _check_contract(pred, tgt):
    B, S = pred.shape[:2]
    for from_closest in (False, True):
        want_d, want_first = _expected(pred, tgt, from_closest)
        r, dist = metrics._rank(pred, tgt, S, from_closest, want_dist=True)
        assert torch.equal(dist, want_d), "dist_out is not sd_cdist of [anchor; pred]"
        assert torch.equal(dist, dist.transpose(1, 2)) and bool((dist.diagonal(dim1=1, dim2=2) == 0).all())
        if from_closest:
            assert r.closest.tolist() == want_first
        dn, idx, score = dist.cpu().numpy(), r.idx.cpu().numpy(), r.score.cpu().numpy()
        for b in range(B):
            picks, scores = R.greedy(dn[b], S)
            assert idx[b].tolist() == picks.tolist(), (b, from_closest)
            assert score[b].tobytes() == scores.tobytes(), (b, from_closest)
        one = metrics.diverse_rank(pred, tgt, 1, from_closest)  # n_choose = 1: the first pick of the full ranking
        assert torch.equal(one.idx, r.idx[:, :1]) and torch.equal(one.score, r.score[:, :1])


@pytest.mark.parametrize("points,features,nseq", [(2, 1, 1), (2, 4800, 37), (64, 9, 37), (64, 36, 1), (65, 1, 37),
                                                  (65, 36, 1), (130, 9, 1), (130, 36, 37), (65, 4800, 1), (130, 4800, 1)])
def test_bitwise_contract(cuda, points, features, nseq):
    g = torch.Generator().manual_seed(points * 10007 + features * 31 + nseq)
    S = points - 1
    tgt = torch.randn(nseq, features, generator=g)
    pred = tgt[:, None] + torch.randn(nseq, S, features, generator=g) * torch.rand(nseq, S, 1, generator=g)
    _check_contract(pred.to(cuda), tgt.to(cuda))


def test_bitwise_contract_unaligned_pred(cuda):
    """pred starts 4 bytes off a 16-byte boundary (features % 4 == 0: only the address keeps the 16-byte loads away)"""
    g = torch.Generator().manual_seed(5)
    B, S, F = 3, 64, 36
    tgt = torch.randn(B, F, generator=g).to(cuda)
    flat = torch.empty(B * S * F + 1, device=cuda)
    pred = flat[1:].view(B, S, F)
    pred.copy_(tgt[:, None] + torch.randn(B, S, F, generator=g).to(cuda))
    assert pred.data_ptr() % 16 == 4 and pred.is_contiguous()
    _check_contract(pred, tgt)
    aligned = metrics.diverse_rank(pred.clone(), tgt, S)
    unaligned = metrics.diverse_rank(pred, tgt, S)
    assert torch.equal(aligned.idx, unaligned.idx) and torch.equal(aligned.score, unaligned.score)


# ---- ties and NaN --------------------------------------------------------------------------------------------
def test_duplicates_resolve_to_the_lower_index(cuda):
    g = torch.Generator().manual_seed(6)
    tgt = torch.zeros(2, 10)
    pred = torch.randn(2, 7, 10, generator=g) * 0.1
    pred[:, 1] = 5.0  # the farthest from the target ...
    pred[:, 4] = pred[:, 1]  # ... and its duplicate
    r = metrics.diverse_rank(pred.to(cuda), tgt.to(cuda), 7)
    assert r.idx[:, 0].tolist() == [1, 1] and r.idx[:, -1].tolist() == [4, 4]
    assert r.score[:, -1].tolist() == [0.0, 0.0]
    assert [sorted(row) for row in r.idx.tolist()] == [list(range(7))] * 2


def test_all_equal_samples_are_picked_in_index_order(cuda):
    pred = torch.full((2, 66, 9), 0.25)
    tgt = torch.zeros(2, 9)
    for fc in (False, True):
        r = metrics.diverse_rank(pred.to(cuda), tgt.to(cuda), 66, from_closest=fc)
        assert r.idx.tolist() == [list(range(66))] * 2
        if fc:
            assert r.closest.tolist() == [0, 0] and bool((r.score == 0).all())


def test_a_nan_sample_is_picked_last(cuda):
    g = torch.Generator().manual_seed(8)
    tgt = torch.randn(3, 12, generator=g)
    pred = tgt[:, None] + torch.randn(3, 40, 12, generator=g)
    pred[0, 0, 3] = pred[1, 17, 0] = pred[2, 39, 11] = float("nan")
    for fc in (False, True):
        r = metrics.diverse_rank(pred.to(cuda), tgt.to(cuda), 40, from_closest=fc)
        idx = r.idx.tolist()
        assert [row[-1] for row in idx] == [0, 17, 39]
        assert [sorted(row) for row in idx] == [list(range(40))] * 3  # every index in range, each once
        assert bool(torch.isnan(r.score[:, -1]).all()) and not bool(torch.isnan(r.score[:, :-1]).any())
        if fc:
            assert all(0 <= c < 40 and c != n for c, n in zip(r.closest.tolist(), (0, 17, 39)))


# ---- CMD ---------------------------------------------------------------------------------------------------------
def test_cmd_accumulator(z, cuda):
    motion, cls, ref = torch.from_numpy(z["cmd_motion"]).to(cuda), z["cmd_cls"], z["cmd_ref"]
    value, per_class, bound = R.cmd_float64(z["cmd_motion"], cls, ref)
    whole = metrics.CMDAccumulator(ref, device=cuda)
    whole.update(motion, torch.from_numpy(cls).to(cuda))
    assert whole.sum.device.type == "cuda" and whole.sum.dtype == torch.float64 and whole.count.dtype == torch.int64
    assert whole.count.tolist() == [4, 4, 0, 3] and whole.total.tolist() == [12]
    got = whole.compute()
    print(f"cmd: device {got!r}, float64 {value!r}, reference {float(z['cmd_value'])!r}, bound {bound:.3e}")
    assert abs(got - value) <= 1e-12 * abs(value)
    assert abs(got - float(z["cmd_value"])) <= bound
    np.testing.assert_allclose(whole.motion_per_class().numpy(), per_class, rtol=1e-12)
    assert torch.equal(whole.motion_per_class()[2], torch.zeros(9, dtype=torch.float64))
    parts = metrics.CMDAccumulator(ref, device=cuda)
    for a in range(0, 12, 4):
        parts.update(motion[a:a + 4], cls[a:a + 4])  # host class indices are copied over
    assert torch.equal(parts.sum, whole.sum) and torch.equal(parts.count, whole.count) and torch.equal(parts.total, whole.total)
    host = metrics.CMDAccumulator(ref)  # the CPU form keeps the kernel's order
    host.update(motion.cpu(), cls)
    assert torch.equal(host.sum, whole.sum.cpu())
    halves = [metrics.CMDAccumulator(ref, device=cuda), metrics.CMDAccumulator(ref, device=cuda)]
    halves[0].update(motion[:6], cls[:6])
    halves[1].update(motion[6:], cls[6:])
    merged = halves[0].merge(halves[1]).compute()
    assert abs(merged - value) <= 1e-12 * abs(value)


def test_cmd_storer_transform(cuda):
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(4, 5, 10, 16, 3, generator=g).to(cuda)
    factory, transform = evaluation.get_cmd_storer(["a", "b", "c"], [0.5, 1.0, 1.5], device=cuda)
    acc = factory(output_transform=None)
    motion, cls = transform(pred=pred, class_idx=[2, 0, 2, 1], target=None)
    assert torch.equal(motion, metrics.motion_for_cmd(pred))
    acc.update(motion, cls)
    value, _, _ = R.cmd_float64(motion.cpu().numpy(), np.array(cls), [0.5, 1.0, 1.5])
    assert abs(acc.compute() - value) <= 1e-12 * abs(value)


# ---- the storers ---------------------------------------------------------------------------------------------
def test_metric_accumulator(z, cuda):
    values = torch.from_numpy(z["storer_values"])
    exact = {"mean": float(values.double().sum() / len(values)), "max": float(values.max()), "min": float(values.min())}
    exact["avg"] = exact["mean"]
    for op in ("mean", "avg", "max", "min"):
        acc = metrics.MetricAccumulator(op)
        for a in range(0, len(values), R.STORER_BATCH):
            acc.update(values[a:a + R.STORER_BATCH].to(cuda))
        assert acc.cumulator.device.type == "cuda" and acc.cumulator.dtype == torch.float64
        got, ref = acc.compute(), float(z[f"storer_{op}"])
        print(f"storer {op}: device {got!r}, float64 {exact[op]!r}, reference {ref!r}")
        assert abs(got - exact[op]) <= 1e-12 * abs(exact[op]), op
        assert abs(got - ref) <= 1e-5 * abs(ref), op
        two = [metrics.MetricAccumulator(op), metrics.MetricAccumulator(op)]
        two[0].update(values[:50].to(cuda))
        two[1].update(values[50:].to(cuda))
        merged = two[0].merge(two[1]).compute()
        assert abs(merged - exact[op]) <= 1e-12 * abs(exact[op]), op
    acc = metrics.MetricAccumulator("max")
    acc.update(torch.from_numpy(z["storer_neg"]).to(cuda))
    assert acc.compute() == float(z["storer_max_neg"]) == 0.0
    acc = metrics.MetricAccumulator("min")
    acc.update(torch.from_numpy(z["storer_big"]).to(cuda))
    assert acc.compute() == float(z["storer_min_big"]) == 1000000.0


def test_metric_set_equals_the_batch_means(cuda, tmp_path):
    g = torch.Generator().manual_seed(10)
    B, S, T, J = 4, 5, 10, 16
    target = torch.randn(B, T, J, 3, generator=g)
    pred = (target[:, None] + 0.1 * torch.randn(B, S, T, J, 3, generator=g)).to(cuda)
    target = target.to(cuda)
    obs = torch.randn(B, 6, J, 3, generator=g).to(cuda)
    mm_gt = [(target[b][None] + 0.05 * torch.randn(1 + b, T, J, 3, generator=g).to(cuda)) for b in range(B)]
    batch = dict(pred=pred, target=target, mm_gt=mm_gt, obs=obs)
    sd = {k: 0.1 * torch.randn(*shape, generator=g) for k, shape in (
        ("recurrent.weight_ih_l0", (384, 48)), ("recurrent.weight_hh_l0", (384, 128)), ("recurrent.bias_ih_l0", (384,)),
        ("recurrent.bias_hh_l0", (384,)), ("recurrent.weight_ih_l1", (384, 128)), ("recurrent.weight_hh_l1", (384, 128)),
        ("recurrent.bias_ih_l1", (384,)), ("recurrent.bias_hh_l1", (384,)), ("linear1.weight", (30, 128)),
        ("linear1.bias", (30,)))}
    torch.save({"model": sd}, tmp_path / "h36m_classifier.pth")
    gt_apd = torch.tensor([1.0, 0.0, 3.0, 2.5], dtype=torch.float64)
    ms = evaluation.metric_set("probabilistic", "h36m16", dataset_split="test", dataset_name="h36m", if_compute_cmd=True,
                               if_compute_fid=True, if_compute_apde=True, device=cuda, classifier_path=str(tmp_path),
                               idx_to_class=["a", "b", "c"], mean_motion_per_class=[0.1, 0.2, 0.3], gt_apd=gt_apd)
    funcs = evaluation.get_stats_funcs("probabilistic", "h36m16")
    assert set(ms.storers) == set(funcs) | {"FID", "CMD", "APDE"}
    ms.update(class_idx=torch.tensor([0, 2, 2, 1]), **batch)
    out = ms.compute()
    assert set(out) == set(ms.storers) and all(isinstance(v, float) for v in out.values())
    for name, fn in funcs.items():
        want = float(fn(**batch).double().mean())
        assert abs(out[name] - want) <= 1e-12 * abs(want), name
    apd = metrics.apd(pred).double().cpu()
    want = float(((apd - gt_apd).abs()[[0, 2, 3]]).mean())  # the segment with gt_APD 0 is skipped
    assert abs(out["APDE"] - want) <= 1e-12 * want
    value, _, _ = R.cmd_float64(metrics.motion_for_cmd(pred).cpu().numpy(), np.array([0, 2, 2, 1]), [0.1, 0.2, 0.3])
    assert abs(out["CMD"] - value) <= 1e-12 * abs(value)
    assert np.isfinite(out["FID"])
    plain = evaluation.metric_set("probabilistic_orig", "h36m16", device=cuda)
    assert set(plain.storers) == {"APD", "ADE", "FDE", "MMADE", "MMFDE"}
    plain.update(**batch)
    plain.update(**batch)  # two equal batches: the same means
    for name, v in plain.compute().items():
        want = float(evaluation.get_stats_funcs("probabilistic_orig", "h36m16")[name](**batch).double().mean())
        assert abs(v - want) <= 1e-12 * abs(want), name
