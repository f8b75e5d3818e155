"""Best-sample selection and mpjpe (skeletondiffusion_amd.metrics.mpjpe / best_sample /
get_best_sample_idx / choose_best_sample, C entry sd_best_sample) against the reference's own outputs
(tests/golden/longterm.npz, made by gen_golden_longterm.py from src/metrics/utils.py:12-30 and
src/metrics/multimodal.py:37-42, run in float64 on the float32 inputs below).

Tolerances: distances at the project's metric tolerance |a-b| <= 1e-5 |b| + 1e-6 (tests/test_metrics.py);
indices, gathered trajectories, masks and tails exact -- the generator asserts that every non-tied
sequence's two smallest distances differ by more than 1e-3 of their value, so the index is not a
rounding question."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from skeletondiffusion_amd import _lib, synthetic

RTOL = 1e-5

# gen_golden_longterm.py:SELECTION_CASES: name -> ((B, S, T, J, 3), pred seed, target seed)
SELECTION_CASES = {
    "tie": ((3, 5, 7, 4, 3), 71, 72),
    "s50": ((2, 50, 20, 16, 3), 73, 74),
    "amass": ((2, 3, 120, 21, 3), 75, 76),
    "s64": ((1, 64, 1, 17, 3), 77, 78),
    "mano": ((2, 1, 5, 51, 3), 79, 80),
}


def selection_inputs(name):
    """gen_golden_longterm.py:selection_inputs restated."""
    shape, sp, st = SELECTION_CASES[name]
    pred = torch.from_numpy(synthetic.normal(shape, seed=sp))
    target = torch.from_numpy(synthetic.normal(shape[:1] + shape[2:], seed=st))
    if name == "tie":
        pred[1, 1] = 0.5 * (pred[1, 1] + target[1])
        pred[1, 3] = pred[1, 1]
    return pred, target


def _close(a, b):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + 1e-6), (a, b)


def ref_selection(pred, target):
    """float64 restatement of metrics/utils.py:12-30 and multimodal.py:37-42:
    (per-sample distances (B, S), idx (B,), best (B, T, J, 3) in pred's dtype)."""
    d = (pred.double() - target.double().unsqueeze(1)).square().sum(-1).sqrt().mean(-1).mean(-1)
    idx = d.min(dim=-1).indices
    return d, idx, pred[torch.arange(pred.shape[0]), idx]


@pytest.mark.parametrize("name", list(SELECTION_CASES))
def test_restatement_matches_reference(name):
    z = golden("longterm")
    pred, target = selection_inputs(name)
    d, idx, best = ref_selection(pred, target)
    _close(d, z[f"{name}_dist"])
    _close(d.min(-1).values, z[f"{name}_mpjpe"])
    assert np.array_equal(idx.numpy(), z[f"{name}_idx"])
    assert np.array_equal(best.numpy(), z[f"{name}_best"])
    if name == "tie":
        assert int(idx[1]) == 1 and torch.equal(pred[1, 1], pred[1, 3])


def test_public_surface_refuses_cpu_tensors():
    from skeletondiffusion_amd import metrics
    from skeletondiffusion_amd._lib import SkelDiffError

    out, y = torch.zeros(2, 3, 4, 5, 3), torch.zeros(2, 4, 5, 3)
    for name in ("mpjpe", "best_sample", "get_best_sample_idx", "choose_best_sample"):
        assert name in metrics.__all__ and callable(getattr(metrics, name))
    with pytest.raises(SkelDiffError):
        metrics.mpjpe(y, out)
    for fn in (metrics.best_sample, metrics.get_best_sample_idx, metrics.choose_best_sample):
        with pytest.raises(SkelDiffError):
            fn(out, y)


def test_host_argument_checks():
    """sd_best_sample validates on the host, before any device call, and names the argument."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)

    def call(nseq=2, samples=5, frames=7, joints=4, coords=3, tail_frames=0, tail_out=None):
        return L.sd_best_sample(p, p, nseq, samples, frames, joints, coords, tail_frames, p, None, None, None,
                                tail_out, None)

    for kw, word in ((dict(samples=65), b"samples"), (dict(samples=0), b"samples"), (dict(coords=2), b"coords"),
                     (dict(tail_frames=8), b"tail_frames"), (dict(tail_frames=-1), b"tail_frames"),
                     (dict(tail_frames=0, tail_out=p), b"tail_out"), (dict(frames=0), b"frames"),
                     (dict(joints=0), b"joints")):
        assert call(**kw) == -1, kw
        assert word in L.sd_last_error(), (kw, L.sd_last_error())
    assert L.sd_best_sample(None, None, 0, 5, 7, 4, 3, 0, None, None, None, None, None, None) == 0


def test_header_declares_entry_point():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bint sd_best_sample\(const float\* pred, const float\* target, int64_t nseq", hdr)
    assert "sd_best_sample" in _lib.EXPORTED and hasattr(_lib.lib(), "sd_best_sample")
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr)


# ---- device ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SELECTION_CASES))
def test_device_selection_matches_reference(cuda, name):
    from skeletondiffusion_amd import metrics as M

    z = golden("longterm")
    pred, target = (t.to(cuda) for t in selection_inputs(name))
    B, S, T = pred.shape[:3]
    per = M.mpjpe(target, pred, reduction="none")
    print(name, "per-sample max relative error",
          float(np.max(np.abs(per.cpu().numpy() - z[f"{name}_dist"]) / z[f"{name}_dist"])))
    _close(per, z[f"{name}_dist"])
    _close(M.mpjpe(target, pred), z[f"{name}_mpjpe"])
    for tail in (None, 1, T):
        idx, dist, best, last = M.best_sample(pred, target, tail=tail)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), z[f"{name}_idx"])
        _close(dist, z[f"{name}_mpjpe"])
        assert best.shape == target.shape and np.array_equal(best.cpu().numpy(), z[f"{name}_best"])
        if tail is None:
            assert last is None
        else:
            assert np.array_equal(last.cpu().numpy(), z[f"{name}_best"][:, T - tail:])
    best, mask = M.get_best_sample_idx(pred, target)
    assert mask.is_cuda and mask.dtype == torch.bool and mask.shape == (B, S)
    onehot = np.zeros((B, S), dtype=bool)
    onehot[np.arange(B), z[f"{name}_idx"]] = True
    assert np.array_equal(mask.cpu().numpy(), onehot) and np.array_equal(best.cpu().numpy(), z[f"{name}_best"])
    best, y = M.choose_best_sample(pred, target)
    assert y is target and np.array_equal(best.cpu().numpy(), z[f"{name}_best"])
    if name == "tie":
        assert int(idx[1]) == 1


def _all_outputs(M, pred, target, tail):
    per = M.mpjpe(target, pred, reduction="none")
    return (per,) + tuple(M.best_sample(pred, target, tail=tail))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tie", "amass", "s64", "mano"])
def test_device_alignment_and_layout(cuda, name):
    """A pred (and target) whose storage starts one, two or three floats into its buffer -- contiguous,
    4-byte aligned only -- and a time-sliced non-contiguous pred give the aligned contiguous copy's
    results bit for bit."""
    from skeletondiffusion_amd import metrics as M

    pred, target = (t.to(cuda) for t in selection_inputs(name))
    T = pred.shape[2]
    tail = max(1, T // 2)
    want = _all_outputs(M, pred, target, tail)

    def shifted(x, k):
        buf = torch.empty(x.numel() + k, device=cuda, dtype=torch.float32)
        v = buf[k:].view(x.shape)
        v.copy_(x)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
        return v

    for kp, kt in ((1, 0), (2, 3), (3, 1), (0, 2)):
        got = _all_outputs(M, shifted(pred, kp), shifted(target, kt), tail)
        for a, b in zip(got, want):
            assert torch.equal(a, b), (name, kp, kt)
    big = torch.randn(pred.shape[0], pred.shape[1], T + 3, *pred.shape[3:], device=cuda)
    big[:, :, 2:2 + T] = pred
    sliced = big[:, :, 2:2 + T]
    assert not sliced.is_contiguous()
    for a, b in zip(_all_outputs(M, sliced, target, tail), want):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_device_determinism_ties_and_nan(cuda):
    from skeletondiffusion_amd import metrics as M

    pred, target = (t.to(cuda) for t in selection_inputs("s50"))
    a, b = _all_outputs(M, pred, target, 4), _all_outputs(M, pred, target, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # a sample and its byte copies get the same bits, also where the copies' blocks start at another
    # 16-byte phase (51 floats per sample: the phase changes from sample to sample)
    p64, t64 = (t.to(cuda) for t in selection_inputs("s64"))
    p64[0, 10] = p64[0, 5]
    p64[0, 11] = p64[0, 5]
    p64[0, 12] = p64[0, 5]
    per = M.mpjpe(t64, p64, reduction="none")
    assert per[0, 5] == per[0, 10] == per[0, 11] == per[0, 12]
    tie_p, tie_t = (t.to(cuda) for t in selection_inputs("tie"))
    per = M.mpjpe(tie_t, tie_p, reduction="none")
    assert per[1, 1] == per[1, 3] and int(M.best_sample(tie_p, tie_t)[0][1]) == 1
    # NaN: torch.min(dim).indices of the per-sample distances, as CPU torch gives it (the first NaN)
    pn = pred.clone()
    pn[0, 30, 3, 2, 1] = float("nan")
    pn[0, 7, 19, 15, 2] = float("nan")
    pn[1, 49, 0, 0, 0] = float("nan")
    per = M.mpjpe(target, pn, reduction="none")
    idx, dist, best, _ = M.best_sample(pn, target)
    want = per.cpu().min(dim=-1).indices
    assert want.tolist() == [7, 49] and torch.equal(idx.cpu(), want)
    assert torch.isnan(dist).all() and torch.isnan(M.mpjpe(target, pn)).all()
    # NaN != NaN: compare the bytes
    assert torch.equal(best.view(torch.int32), pn[torch.arange(2, device=cuda), idx].view(torch.int32))


@pytest.mark.gpu
def test_device_edges(cuda):
    from skeletondiffusion_amd import metrics as M
    from skeletondiffusion_amd._lib import SkelDiffError

    empty = M.best_sample(torch.zeros(0, 5, 7, 4, 3, device=cuda), torch.zeros(0, 7, 4, 3, device=cuda), tail=2)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 7, 4, 3), (0, 2, 4, 3)]
    pred, target = (t.to(cuda) for t in selection_inputs("tie"))
    with pytest.raises(SkelDiffError):
        M.best_sample(pred, target, tail=8)  # more than the 7 frames
    with pytest.raises(SkelDiffError):
        M.mpjpe(torch.zeros(2, 7, 4, 2, device=cuda), torch.zeros(2, 65, 7, 4, 2, device=cuda))
    with pytest.raises(ValueError):
        M.mpjpe(target[:, :6], pred)
