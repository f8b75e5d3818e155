"""The validation metrics of the two training loops (reference src/train_utils.py:56-135): the limb-length
statistics of src/metrics/body_realism.py:4-107 and the per-frame MPJPE / FDE metric classes
(ignite_mpjpe.py, ignite_fde.py).  tests/golden/validation.npz (made by gen_golden_validation.py from the
reference's own functions and classes, in float64 on float32 inputs) against a float64 restatement kept
here; the host side of the new C entries (argument refusals, the ABI number) and of the accumulators
(states on the CPU).  CPU only: the device tests are in tests/test_gpu_validation_metrics.py, which
compares against this fixture and this restatement.

Tolerance: the project's metric tolerance of tests/test_metrics_realism.py, |a - b| <= 1e-5 |b| + 1e-6; on
the near-rigid case the relative term alone; NaN positions equal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from skeletondiffusion_amd import _lib, synthetic
from test_metrics_realism import RTOL, _atol, _close, _limb_len

CASES = ["normal", "rigid", "amass21", "mano51", "freeman17", "T2", "T1"]
MODES = ("mean", "max", "min", "none")
LONG_KEYS = ("long_mpjpe_table", "long_mpjpe_joint_table", "long_mpjpe_mean", "long_mpjpe_joint_mean", "long_fde",
             "long_best_mpjpe_table", "long_best_fde")


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


def cases():
    """gen_golden_validation.py:cases, restated: name -> (skeleton, pred, target)."""
    rest = N((2, 1, 1, 16, 3), 53) * 0.3
    c = {
        "normal": ("h36m16", N((2, 7, 20, 16, 3), 51), N((2, 20, 16, 3), 52)),
        "rigid": ("h36m16", rest + 1e-2 * N((2, 7, 20, 16, 3), 54), rest[:, 0] + 1e-3 * N((2, 20, 16, 3), 55)),
        "amass21": ("amass21", N((2, 5, 33, 21, 3), 56), N((2, 33, 21, 3), 57)),
        "mano51": ("mano51", N((1, 3, 4, 51, 3), 58), N((1, 4, 51, 3), 59)),
        "freeman17": ("freeman17", N((1, 2, 5, 17, 3), 60), N((1, 5, 17, 3), 61)),
    }
    _, pred, target = c["normal"]
    c["T2"] = ("h36m16", pred[:, :, :2], target[:, :2])
    c["T1"] = ("h36m16", pred[:, :, :1], target[:, :1])
    return c


def long_case():
    """gen_golden_validation.py:long_case: (pred (11, 3, 61, 16, 3), target (11, 61, 16, 3))."""
    return N((11, 3, 61, 16, 3), 63), N((11, 61, 16, 3), 64)


def expected_keys(frames):
    """The fixture's keys of a case: the reference raises on max / min of the jitter of a single frame."""
    keys = []
    for mode in MODES:
        jitter_ok = frames > 1 or mode in ("mean", "none")
        for tag in ((mode,) if mode == "none" else (mode, mode + "_ps")):
            keys.append(f"variance_{tag}")
            if jitter_ok:
                keys.append(f"jitter_{tag}")
        if mode != "none":
            keys.append(f"error_{mode}")
        if jitter_ok:
            keys.append(f"wrtgt_{mode}")
    return keys


# ---- float64 restatement -------------------------------------------------------------------------------
def _over(v, mode, dims):
    """`mode` over the trailing `dims` axes, one after the other (max / min keep NaN, as torch's)."""
    for _ in range(dims):
        v = v.mean(-1) if mode == "mean" else (v.max(-1).values if mode == "max" else v.min(-1).values)
    return v


def R_limb(pred, target, limbseq):
    """Every quantity of the fixture (keys as gen_golden_validation.py:all_metrics) in float64.  The variance is
    the mean squared deviation from the mean length, never E[x^2] - mean^2."""
    pred, target = pred.double(), target.double()
    T = pred.shape[2]
    ll, tl = _limb_len(pred, limbseq), _limb_len(target, limbseq)      # (B, S, T, L), (B, T, L)
    var = ((ll - ll.mean(-2, keepdim=True)) ** 2).sum(-2) / (T - 1)     # (B, S, L); T == 1: 0 / 0
    jit = (ll[:, :, 1:] - ll[:, :, :-1]).abs()                          # (B, S, T - 1, L)
    tjit = (tl[:, 1:] - tl[:, :-1]).abs()[:, None]                      # (B, 1, T - 1, L)
    err = (tl[:, None] - ll).abs().mean(-1).mean(-1)                    # (B, S)
    out = {"variance_none": var, "jitter_none": jit, "wrtgt_none": jit - tjit}
    for mode in MODES[:3]:
        out[f"variance_{mode}_ps"], out[f"variance_{mode}"] = _over(var, mode, 1), _over(var, mode, 2)
        out[f"error_{mode}"] = _over(err, mode, 1)
        if T > 1 or mode == "mean":
            js, jt = _over(jit, mode, 2), _over(tjit, mode, 2)      # (B, S), (B, 1)
            out[f"jitter_{mode}_ps"], out[f"jitter_{mode}"] = js, _over(js, mode, 1)
            # body_realism.py:21-29: the (B,) values are reduced once more over their last axis, the batch
            out[f"wrtgt_{mode}"] = (_over(_over(js, mode, 1), mode, 1) - _over(_over(jt, mode, 1), mode, 1)).unsqueeze(0)
    return out


def R_frame_error(pred, target, idx=None):
    """(T, J) float64: the mean over the rows of ||pred[r, idx[r]] - target[r]|| per frame and joint; pred
    (R, S, T, J, 3) (sample 0 without idx).  An index that is no sample makes the row NaN."""
    pred, target = pred.double(), target.double()
    R, S = pred.shape[:2]
    idx = torch.zeros(R, dtype=torch.int64) if idx is None else torch.as_tensor(idx).cpu()
    e = (pred[torch.arange(R), idx.clamp(0, S - 1)] - target).norm(dim=-1)
    e[(idx < 0) | (idx >= S)] = float("nan")
    return e.mean(0)


def R_best_idx(pred, target):
    """metrics/utils.py:14: the sample closest to the target."""
    return (pred.double() - target.double().unsqueeze(1)).norm(dim=-1).mean(-1).mean(-1).min(dim=-1).indices


def R_table(profile):
    return profile[[t for t in range(0, 16 * 30, 30) if t < profile.shape[0]]]


def R_long(pred, target):
    """The long case's keys from R_frame_error."""
    first, best = R_frame_error(pred, target), R_frame_error(pred, target, R_best_idx(pred, target))
    return {"long_mpjpe_table": R_table(first.mean(-1)), "long_mpjpe_joint_table": R_table(first),
            "long_mpjpe_mean": first.mean(-1).mean(0), "long_mpjpe_joint_mean": first.mean(0), "long_fde": first[-1].mean(),
            "long_best_mpjpe_table": R_table(best.mean(-1)), "long_best_fde": best[-1].mean()}


# ---- the fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    """Every function x mode x if_per_sample of the seven cases: J = 16 ("normal" and near-rigid), 21, 51, 17, and
    the T = 2 / T = 1 edges (NaN variance and jitter mean, an empty 'none' jitter, as the reference gives)."""
    z = golden("validation")
    skel, pred, target = cases()[name]
    got = R_limb(pred, target, z[f"{skel}_limbseq"].tolist())
    keys = expected_keys(pred.shape[2])
    stored = [k for k in z.files if k.startswith(name + "_") and not k.endswith("_limbseq")]
    assert sorted(stored) == sorted(f"{name}_{k}" for k in keys)
    assert sorted(got) == sorted(keys)  # every quantity is compared, none skipped
    for k in keys:
        _close(got[k], z[f"{name}_{k}"], _atol(name))
    if name == "T1":
        assert np.isnan(z["T1_variance_none"]).all() and np.isnan(z["T1_jitter_mean"]).all()
        assert z["T1_jitter_none"].shape == (2, 7, 0, 16) and z["T1_wrtgt_mean"].shape == (1,)
    if name == "normal":
        assert z["normal_wrtgt_max"].shape == (1,) and z["normal_wrtgt_none"].shape == (2, 7, 19, 16)


def test_metric_classes_of_the_long_case():
    """MeanPerJointPositionError (every keep_time_dim / keep_joint_dim) and FinalDisplacementError fed in three
    uneven batches, of sample 0 and of the best sample; the time table has rows 0, 30, 60."""
    z = golden("validation")
    assert z["long_batches"].tolist() == [5, 2, 4]
    got = R_long(*long_case())
    assert sorted(got) == sorted(LONG_KEYS)
    for k in LONG_KEYS:
        _close(got[k], z[k])
    assert z["long_mpjpe_table"].shape == (3,) and z["long_mpjpe_joint_table"].shape == (3, 16)
    assert z["long_mpjpe_joint_mean"].shape == (16,) and z["long_fde"].shape == ()


def test_one_pass_variance_misses_the_rigid_case():
    """The near-rigid case does what it is there for: float32 E[x^2] - mean^2 of raw lengths misses the relative
    tolerance by orders of magnitude."""
    z = golden("validation")
    skel, pred, _ = cases()["rigid"]
    ll = _limb_len(pred, z[f"{skel}_limbseq"].tolist())  # float32
    T = ll.shape[2]
    one_pass = ((ll ** 2).mean(-2) - ll.mean(-2) ** 2) * (T / (T - 1))
    ref = z["rigid_variance_none"]
    assert (np.abs(one_pass.double().numpy() - ref) / np.abs(ref)).max() > 100 * RTOL


def test_limb_tables_equal_the_package():
    from skeletondiffusion_amd import skeletons

    z = golden("validation")
    for skel in ("h36m16", "amass21", "freeman17", "mano51"):
        assert np.array_equal(np.asarray(skeletons.limbseq(skel)), z[f"{skel}_limbseq"])


# ---- the C entries: header, binding, argument refusals ---------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bint sd_limb_stats\(const float\* pred, const float\* target, int64_t nseq", hdr)
    assert re.search(r"\bint sd_frame_error_update\(const float\* pred, const float\* target, const int64_t\* idx", hdr)
    for name in ("sd_limb_stats", "sd_frame_error_update"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4


def _i32(rows):
    flat = [int(v) for r in rows for v in r]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat)


def test_host_argument_checks():
    """sd_limb_stats / sd_frame_error_update validate on the host, before any device call, and name the argument."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)
    limbs3 = [[0, 1], [1, 2], [2, 3]]

    def limb_call(nseq=2, samples=5, frames=7, joints=4, limbs=limbs3, nlimbs=None, target=None, scratch=None, seq=None,
                  diff=None):
        return L.sd_limb_stats(p, target, nseq, samples, frames, joints, _i32(limbs) if limbs is not None else None,
                               len(limbs) if nlimbs is None else nlimbs, p, None, scratch, seq, None, diff, None)

    for kw, word in ((dict(nseq=-1), b"nseq"), (dict(samples=0), b"samples"), (dict(samples=65), b"samples"),
                     (dict(frames=0), b"frames"), (dict(joints=0), b"joints"), (dict(joints=65), b"joints"),
                     (dict(nlimbs=0), b"nlimbs"), (dict(nlimbs=65, limbs=[[0, 1]] * 65), b"nlimbs"),
                     (dict(limbs=None, nlimbs=3), b"limbseq"), (dict(limbs=[[0, 1], [1, 4], [2, 3]]), b"limbseq[1]"),
                     (dict(limbs=[[-1, 1], [1, 2], [2, 3]]), b"limbseq[0]"), (dict(seq=p), b"sample_scratch"),
                     (dict(diff=p), b"target")):
        assert limb_call(**kw) == -1, kw
        assert word in L.sd_last_error(), (kw, L.sd_last_error())
    assert L.sd_limb_stats(None, None, 0, 5, 7, 4, _i32(limbs3), 3, *([None] * 7)) == 0  # nseq == 0: nothing to do
    assert L.sd_limb_stats(None, None, 2, 5, 7, 4, _i32(limbs3), 3, p, *([None] * 6)) == -1 and b"pred" in L.sd_last_error()

    def frame_call(rows=3, samples=5, frames=7, joints=4, frame0=0, nframes=7, idx=p, sum_=p, count=p, pred=p, target=p):
        return L.sd_frame_error_update(pred, target, idx, rows, samples, frames, joints, frame0, nframes, sum_, count, None)

    for kw, word in ((dict(rows=-1), b"rows"), (dict(samples=0), b"samples"), (dict(samples=65), b"samples"),
                     (dict(idx=None), b"idx"), (dict(frames=0), b"frames"), (dict(joints=0), b"joints"),
                     (dict(joints=65), b"joints"), (dict(frame0=-1), b"frame0"), (dict(frame0=7, nframes=1), b"frame0"),
                     (dict(nframes=0), b"nframes"), (dict(frame0=3, nframes=5), b"nframes"), (dict(sum_=None), b"sum"),
                     (dict(count=None), b"count"), (dict(pred=None), b"pred"), (dict(target=None), b"target")):
        assert frame_call(**kw) == -1, kw
        assert word in L.sd_last_error(), (kw, L.sd_last_error())
    assert frame_call(rows=0, pred=None, target=None, idx=None, samples=1) == 0  # rows == 0: nothing to do


# ---- the Python surface on the host --------------------------------------------------------------------------
def test_public_surface_refuses_cpu_tensors_and_unknown_modes():
    from skeletondiffusion_amd import evaluation as E, metrics as M, skeletons
    from skeletondiffusion_amd._lib import SkelDiffError

    names = ("limb_length_variance", "limb_length_jitter", "limb_length_error", "limb_length_variation_difference_wrtGT",
             "limb_stats", "format_metric_time_table", "MPJPEAccumulator", "FDEAccumulator")
    for name in names:
        assert name in M.__all__ and callable(getattr(M, name)), name
    pred, target, ls = torch.zeros(2, 3, 4, 16, 3), torch.zeros(2, 4, 16, 3), skeletons.limbseq("h36m16")
    for call in (lambda: M.limb_length_variance(pred, ls), lambda: M.limb_length_variance(pred, ls, mode="none"),
                 lambda: M.limb_length_jitter(pred, ls, if_per_sample=True), lambda: M.limb_length_error(target, pred, ls),
                 lambda: M.limb_length_variation_difference_wrtGT(target, pred, ls), lambda: M.limb_stats(pred, ls, target)):
        with pytest.raises(SkelDiffError):
            call()
    for call in (lambda: M.limb_length_variance(pred, ls, mode="std"), lambda: M.limb_length_jitter(pred, ls, mode="avg"),
                 lambda: M.limb_length_error(target, pred, ls, mode="none"),
                 lambda: M.limb_length_variation_difference_wrtGT(target, pred, ls, mode="median")):
        with pytest.raises(ValueError, match="mode"):
            call()
    for mode in ("max", "min"):  # the reference's max over an empty axis raises
        with pytest.raises(ValueError, match="frames"):
            M.limb_length_jitter(pred[:, :, :1], ls, mode=mode)
    assert "validation_set" in E.__all__
    with pytest.raises(ValueError, match="kind"):
        E.validation_set("classifier", "h36m16")
    with pytest.raises(KeyError):
        E.validation_set("diffusion", "mano52")  # no limb table
    assert set(E.validation_set("autoencoder", "h36m16", device="cpu").storers) == {"MPJPE", "ADE", "FDE"}
    assert set(E.validation_set("diffusion", "h36m16", loss_fn=lambda a, b: (a - b).abs().mean(), device="cpu").storers) \
        == {"MPJPE", "APD", "ADE", "LLVar", "Loss"}


def test_time_table():
    from skeletondiffusion_amd import metrics as M

    for frames, rows in ((1, [0]), (30, [0]), (31, [0, 30]), (61, [0, 30, 60]), (100, [0, 30, 60, 90]), (600, list(range(0, 480, 30)))):
        prof = torch.arange(frames, dtype=torch.float64)
        assert M.format_metric_time_table(prof).tolist() == [float(r) for r in rows]
    assert M.format_metric_time_table(torch.zeros(61, 16)).shape == (3, 16)


def _feed(acc, pred, target, batches, **kw):
    r0 = 0
    for n in batches:
        acc.update(pred[r0:r0 + n], target[r0:r0 + n], **kw)
        r0 += n
    return acc


def test_accumulators_on_the_host():
    """States on the CPU: the three uneven batches of the fixture's long case, every keep_* setting, the best
    sample, merge, reset and compute before any update."""
    from skeletondiffusion_amd import metrics as M
    from skeletondiffusion_amd._lib import SkelDiffError

    z = golden("validation")
    pred, target = long_case()
    batches = z["long_batches"].tolist()
    first = pred[:, 0]
    for key, kw in (("long_mpjpe_table", {}), ("long_mpjpe_joint_table", dict(keep_joint_dim=True)),
                    ("long_mpjpe_mean", dict(keep_time_dim=False)),
                    ("long_mpjpe_joint_mean", dict(keep_time_dim=False, keep_joint_dim=True))):
        acc = M.MPJPEAccumulator(**kw)
        with pytest.raises(SkelDiffError, match="at least one example"):
            acc.compute()
        out = _feed(acc, first, target, batches).compute()
        assert out.dtype == torch.float64 and out.device.type == "cpu"
        _close(out, z[key])
    fde = M.FDEAccumulator()
    with pytest.raises(SkelDiffError, match="at least one example"):
        fde.compute()
    _close(_feed(fde, first, target, batches).compute(), z["long_fde"])
    assert tuple(fde.sum.shape) == (1, 16) and int(fde.count) == 11
    _close(_feed(M.MPJPEAccumulator(), pred, target, batches, best=True).compute(), z["long_best_mpjpe_table"])
    _close(_feed(M.FDEAccumulator(), pred, target, batches, idx=None, best=True).compute(), z["long_best_fde"])
    idx = R_best_idx(pred, target)
    by_idx = M.MPJPEAccumulator()
    by_idx.update(pred, target, idx=idx)
    _close(by_idx.compute(), z["long_best_mpjpe_table"])

    # merge of two halves = one accumulator over all rows (sums of the same rows, another order: not bitwise)
    a, b = M.MPJPEAccumulator(), M.MPJPEAccumulator()
    a.update(first[:5], target[:5])
    b.update(first[5:], target[5:])
    assert int(a.merge(b).count) == 11
    _close(a.compute(), z["long_mpjpe_table"])
    # the row-ordered sums do not depend on the split into calls
    one, many = M.MPJPEAccumulator(), M.MPJPEAccumulator()
    one.update(first, target)
    _feed(many, first, target, [1] * 11)
    assert torch.equal(one.sum, many.sum)
    a.reset()
    assert a.sum is None and int(a.count) == 0
    with pytest.raises(SkelDiffError):
        a.compute()
    # refusals: several samples without a choice, both choices, another shape after the first batch, a wrong idx count
    acc = M.MPJPEAccumulator()
    with pytest.raises(ValueError, match="samples"):
        acc.update(pred, target)
    with pytest.raises(ValueError, match="not both"):
        acc.update(pred, target, idx=idx, best=True)
    with pytest.raises(ValueError, match="indices"):
        acc.update(pred, target, idx=idx[:3])
    acc.update(first, target)
    with pytest.raises(ValueError, match="after batches"):
        acc.update(first[:, :30], target[:, :30])
    # an index that is no sample: that row is NaN in all its sums, as on the device
    bad = M.FDEAccumulator()
    bad.update(pred[:2], target[:2], idx=torch.tensor([1, 3]))
    assert torch.isnan(bad.sum).all() and int(bad.count) == 2
