"""FID on the device (metrics.FIDClassifier / FIDAccumulator; C entries sd_fid_features, sd_fid_stats_update;
DESIGN.md §4p) against tests/golden/fid.npz -- the reference's own float32 activations and fid() values -- and
against the float64 restatement of tests/test_fid.py.

Tolerances.  Features: 2e-5 absolute, against the fixture and against float64: the bar tests/test_gpu_kernels.py
holds kernels to, about 30x the reference's own float32 drift on these cases (1.5e-7 .. 7.3e-7).  Statistics:
1e-9 of the largest entry (float64 sums of float32 products, at most a few thousand terms).  End to end: 1e-4
relative against the reference's fid(): a worst-sign 1e-4 perturbation of every reference pred activation moves
the reference's FID by 1.4e-4 relative on `short`, so features inside 2e-5 move it by about 3e-5."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import _lib, evaluation, metrics, synthetic
from skeletondiffusion_amd._lib import SkelDiffError
from test_fid import CASES, FEAT, H, R_features, fid_inputs, fid_state_dict, restated, state_of

pytestmark = pytest.mark.gpu
TOL = 2e-5
TILE = 32  # sd_fid.hip kTile


@functools.lru_cache(maxsize=None)
def classifier(J=16):
    return metrics.FIDClassifier(fid_state_dict(J), "cuda:0")


def _err(tag, got, ref):
    e = float(np.abs(got.detach().cpu().double().numpy() - np.asarray(ref, dtype=np.float64)).max())
    print(f"{tag}: max abs error {e:.2e}")
    return e


def _features_null_h0(c, x):
    """sd_fid_features with h0 == NULL (zeros), which the Python surface never passes."""
    rows, frames = x.shape[0], x.shape[1]
    L = _lib.lib()
    ws = torch.empty(L.sd_fid_workspace_bytes(ctypes.byref(c._desc), rows), device=x.device, dtype=torch.uint8)
    out = torch.empty(rows, c.feat_size, device=x.device)
    _lib.check(L.sd_fid_features(ctypes.byref(c._desc), x.data_ptr(), rows, frames, None, out.data_ptr(), ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream(x.device).cuda_stream))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_activations(name, cuda):
    (B, S, T, J), _ = CASES[name]
    z = golden("fid")
    pred, target, hp, hg = (t.to(cuda) for t in fid_inputs(B, S, T, J))
    c = classifier(J)
    rp, rg = restated(name)
    for tag, x, h, ref, r64 in (("pred", pred, hp, z[f"{name}_pred_act"], rp), ("gt", target, hg, z[f"{name}_gt_act"], rg)):
        got = c.features(x, h)  # (..., T, J, 3) as stored
        assert got.shape == ref.shape and got.dtype == torch.float32
        assert _err(f"{name} {tag} vs reference", got, ref) < TOL
        assert _err(f"{name} {tag} vs float64", got, r64) < TOL
        # the reference's call: (b, input_size, frames), the permuted view of fid.py:113 / :117
        flat = x.reshape(-1, T, 3 * J)
        again = c.get_fid_features(motion_sequence=flat.permute(0, 2, 1), hidden_unit=h)
        assert torch.equal(again, got)
        assert torch.equal(c.features(flat, h), got)  # (rows, frames, input_size)


@pytest.mark.parametrize("rows", [1, TILE - 1, TILE + 1, 67])
def test_ragged_tiles(rows, cuda):
    c, sd = classifier(16), fid_state_dict(16)
    for frames in (1, 2, 7):
        x = 0.4 * torch.from_numpy(synthetic.normal((rows, frames, 48), 200 + frames))
        h0 = torch.from_numpy(synthetic.normal((2, rows, H), 300 + frames))
        got = c.features(x.to(cuda), h0.to(cuda))
        assert _err(f"rows {rows} frames {frames} h0", got, R_features(sd, x, h0)) < TOL
        got0 = _features_null_h0(c, x.to(cuda))
        assert _err(f"rows {rows} frames {frames} h0 NULL", got0, R_features(sd, x, None)) < TOL
        assert torch.equal(got0, c.features(x.to(cuda), torch.zeros(2, rows, H, device=cuda)))


def test_rows_do_not_depend_on_their_batch(cuda):
    """Bitwise: rows 5..20 alone (tile rows 0..15) and inside a 67-row call (tile rows 5..20)."""
    c = classifier(16)
    x = (0.4 * torch.from_numpy(synthetic.normal((67, 7, 16, 3), 210))).to(cuda)
    h0 = torch.from_numpy(synthetic.normal((2, 67, H), 211)).to(cuda)
    full = c.features(x, h0)
    alone = c.features(x[5:21].contiguous(), h0[:, 5:21].contiguous())
    assert torch.equal(alone, full[5:21])
    late = c.features(x[40:].contiguous(), h0[:, 40:].contiguous())  # another tile, another offset
    assert torch.equal(late, full[40:])


def _check_state(tag, state, feats):
    """A device state against the float64 statistics of the same float32 features on the host."""
    a = feats.detach().cpu().numpy()
    ref = state_of(a)
    st = state.cpu()
    scale = float(ref[1:].abs().max())
    err = float((st - ref).abs().max())
    print(f"{tag}: max |state - host float64| = {err:.2e} (largest entry {scale:.3e})")
    assert float(st[0]) == a.shape[0] and err <= 1e-9 * scale
    mu, sigma = metrics.FIDAccumulator.statistics(st)
    cov = np.cov(a, rowvar=False)
    assert np.abs(sigma.numpy() - cov).max() <= 1e-9 * np.abs(cov).max()
    assert mu.dtype == torch.float32
    assert np.abs(mu.double().numpy() - np.mean(a.astype(np.float64), axis=0)).max() <= 6e-8  # one float32 rounding of |mu| < 1


def test_statistics_three_uneven_updates(cuda):
    c = classifier(16)
    x = (0.4 * torch.from_numpy(synthetic.normal((67, 7, 48), 220))).to(cuda)
    h0 = torch.from_numpy(synthetic.normal((2, 67, H), 221)).to(cuda)
    feats = c.features(x, h0)

    def three():
        acc = metrics.FIDAccumulator(c)
        for lo, hi in ((0, 7), (7, 40), (40, 67)):
            acc.update_features(pred_feats=feats[lo:hi])
        return acc.state_pred.clone()

    st = three()
    _check_state("7 + 33 + 27 rows", st, feats)
    one = metrics.FIDAccumulator(c)
    one.update_features(pred_feats=feats)
    _check_state("one call", one.state_pred, feats)
    assert float((one.state_pred - st).abs().max()) <= 1e-9 * float(st[1:].abs().max())
    assert torch.equal(three(), st)  # bitwise run to run
    assert float(one.state_gt.abs().max()) == 0.0


def test_statistics_over_several_chunks(cuda):
    """More rows than one workgroup's 256-row chunk, a ragged last chunk, feat below 30."""
    for feat, parts in ((FEAT, (7, 333, 260)), (5, (600,)), (32, (257, 1))):
        rows = sum(parts)
        feats = torch.from_numpy(synthetic.uniform((rows, feat), 230 + feat)).to(cuda)
        acc = metrics.FIDAccumulator(feat_size=feat, device=cuda)
        lo = 0
        for n in parts:
            acc.update_features(gt_feats=feats[lo:lo + n])
            lo += n
        _check_state(f"feat {feat} rows {parts}", acc.state_gt, feats)


@pytest.mark.parametrize("name", [n for n, (_, f) in CASES.items() if f])
def test_fid_end_to_end_two_batches(name, cuda):
    (B, S, T, J), _ = CASES[name]
    ref = float(golden("fid")[f"{name}_fid"])
    pred, target, hp, hg = (t.to(cuda) for t in fid_inputs(B, S, T, J))
    acc = metrics.FIDAccumulator(classifier(J))
    cut = B // 2 + 1
    for lo, hi in ((0, cut), (cut, B)):
        acc.update(pred[lo:hi], target[lo:hi], hp[:, lo * S:hi * S], hg[:, lo:hi])
    got = acc.compute()
    print(f"{name}: FID {got:.9f}, reference {ref:.9f}, relative {abs(got - ref) / ref:.2e}")
    assert isinstance(got, float) and abs(got - ref) <= 1e-4 * ref
    acc.reset()
    with pytest.raises(ValueError, match="at least 2 rows"):
        acc.compute()


def test_default_hidden_state_is_torch_randn_pred_first(cuda):
    B, S, T, J = 3, 2, 4, 16
    pred, target, _, _ = (t.to(cuda) for t in fid_inputs(B, S, T, J))
    c = classifier(J)
    torch.manual_seed(77)
    a = metrics.FIDAccumulator(c)
    a.update(pred, target)
    torch.manual_seed(77)
    hp = torch.randn(2, B * S, H, device=cuda)
    hg = torch.randn(2, B, H, device=cuda)
    b = metrics.FIDAccumulator(c)
    b.update(pred, target, hp, hg)
    assert torch.equal(a.state_pred, b.state_pred) and torch.equal(a.state_gt, b.state_gt)
    torch.manual_seed(77)
    assert torch.equal(c.features(pred), c.features(pred, hp))


def test_cpu_tensors_raise(cuda):
    c = classifier(16)
    with pytest.raises(SkelDiffError):
        c.features(torch.zeros(2, 3, 16, 3))
    with pytest.raises(SkelDiffError):
        c.features(torch.zeros(2, 3, 16, 3, device=cuda), torch.zeros(2, 2, H))
    with pytest.raises(SkelDiffError):
        metrics.FIDAccumulator(c).update_features(pred_feats=torch.zeros(4, FEAT))


def test_get_fid_storer(tmp_path, cuda):
    torch.save({"model": dict(fid_state_dict(16))}, tmp_path / "h36m_classifier.pth")
    with pytest.raises(AssertionError):
        evaluation.get_fid_storer(classifier_path=str(tmp_path), if_consider_hip=True)
    acc, select = evaluation.get_fid_storer(precomputed_folder=str(tmp_path), if_consider_hip=False, device=cuda)
    (B, S, T, J), _ = CASES["short"]
    pred, target, hp, hg = (t.to(cuda) for t in fid_inputs(B, S, T, J))
    p, t = select(pred=pred, target=target, mm_gt=None)
    acc.update(p, t, hp, hg)
    ref = float(golden("fid")["short_fid"])
    assert abs(acc.compute() - ref) <= 1e-4 * ref
