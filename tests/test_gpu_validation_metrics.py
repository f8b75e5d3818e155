"""On-device validation metrics (skeletondiffusion_amd.metrics.limb_stats and the reference-signature functions
built on it, MPJPEAccumulator / FDEAccumulator, evaluation.validation_set; C entries sd_limb_stats /
sd_frame_error_update) against tests/golden/validation.npz -- the reference's own functions and
metric classes run in float64 -- and against the float64 restatement of tests/test_validation_metrics.py.

Tolerance: the project's metric tolerance, |a - b| <= 1e-5 |b| + 1e-6, the relative term alone on the near-rigid
case; NaN patterns equal.  The device forms limb lengths, per-joint distances and every sum in float64 and rounds
the results to float32 once (6e-8), far inside the bound, so it is not widened for any shape here.  The batching
test asks for equal bits."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import _lib, synthetic
from test_metrics_realism import _atol, _close
from test_validation_metrics import (CASES, LONG_KEYS, MODES, R_best_idx, R_frame_error, R_limb, R_long, R_table, cases,
                                     expected_keys, long_case)

pytestmark = pytest.mark.gpu
SKEL_BY_J = {16: "h36m16", 21: "amass21", 17: "freeman17", 51: "mano51"}


def N(shape, seed, scale=1.0):
    return torch.from_numpy(synthetic.normal(shape, seed=seed)) * scale


def _limbseq(J):
    from skeletondiffusion_amd import skeletons

    return skeletons.limbseq(SKEL_BY_J[J])


def _single(M, p, g, limbseq, keys):
    """The fixture's keys from the reference-signature functions."""
    out = {}
    for k in keys:
        what, _, tag = k.partition("_")
        mode, ps = (tag[:-3], True) if tag.endswith("_ps") else (tag, False)
        if what == "variance":
            out[k] = M.limb_length_variance(p, limbseq, mode=mode, if_per_sample=ps)
        elif what == "jitter":
            out[k] = M.limb_length_jitter(p, limbseq, mode=mode, if_per_sample=ps)
        elif what == "error":
            out[k] = M.limb_length_error(g, p, limbseq, mode=mode)
        else:
            out[k] = M.limb_length_variation_difference_wrtGT(g, p, limbseq, mode=mode)
    return out


def _fused(r, keys):
    """The fixture's keys that `LimbStats` holds (everything but the ..._wrtGT differences)."""
    out = {}
    for k in keys:
        if not k.startswith("wrtgt"):
            out[k] = getattr(r, k[:-3] + "_persample" if k.endswith("_ps") else k)
    return out


def _same_bits(a, b):
    """Equal, NaN for NaN."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _check(tag, got, ref, atol=1e-6):
    for k, v in got.items():
        a, b = np.asarray(v.detach().cpu(), dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        ok = ~np.isnan(b) & (b != 0)
        rel = float(np.max(np.abs(a - b)[ok] / np.abs(b)[ok])) if ok.any() else 0.0
        print(f"{tag} {k}: max relative error {rel:.3e}")
        _close(v, ref[k], atol)


@functools.lru_cache(maxsize=None)
def _restated(B, S, T, J, seed, L=None):
    """Seeded inputs of a shape with its skeleton's limb table (cut to L limbs) and the float64 restatement, once."""
    limbseq = _limbseq(J)[:L]
    pred, target = N((B, S, T, J, 3), seed), N((B, T, J, 3), seed + 1)
    return pred, target, limbseq, R_limb(pred, target, limbseq)


# ---- limb statistics: the fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_case(cuda, name):
    """Every function x mode x if_per_sample of the seven fixture cases, from the fused call and from the
    reference-signature functions; at T = 1 NaN where the reference gives NaN and ValueError where it raises."""
    from skeletondiffusion_amd import metrics as M

    z = golden("validation")
    skel, pred, target = cases()[name]
    limbseq = z[f"{skel}_limbseq"].tolist()
    p, g = pred.to(cuda), target.to(cuda)
    keys = expected_keys(pred.shape[2])
    ref = {k: z[f"{name}_{k}"] for k in keys}
    single = _single(M, p, g, limbseq, keys)
    assert sorted(single) == sorted(keys)
    _check(name, single, ref, _atol(name))
    r = M.limb_stats(p, limbseq, g)
    _check(name + " fused", _fused(r, keys), ref, _atol(name))
    B, S, T = pred.shape[:3]
    assert r.jitter_mean_limb.shape == r.error_limb.shape == (B, S, len(limbseq)) and r.jitter_none.shape[2] == T - 1
    if name == "T1":
        for mode in ("max", "min"):
            with pytest.raises(ValueError, match="frames"):
                M.limb_length_jitter(p, limbseq, mode=mode)
            with pytest.raises(ValueError, match="frames"):
                M.limb_length_variation_difference_wrtGT(g, p, limbseq, mode=mode)
        assert torch.isnan(r.variance_none).all() and torch.isnan(r.jitter_max).all() and not torch.isnan(r.error_mean).any()
    for call in (lambda: M.limb_length_variance(p, limbseq, mode="std"), lambda: M.limb_length_error(g, p, limbseq, mode="none")):
        with pytest.raises(ValueError, match="mode"):
            call()
    no_target = M.limb_stats(p, limbseq)
    assert no_target.error_mean is None and _same_bits(no_target.variance_none, r.variance_none)


# ---- limb statistics: shapes where the kernel can still go wrong -------------------------------------------------------
# frames = one staged tile + 1 (32 + 1 up to J = 21, 13 + 1 at J = 51), two tiles + 1, 1 and 64 samples
@pytest.mark.parametrize("B,S,T,J", [(2, 1, 33, 16), (1, 64, 33, 21), (2, 3, 14, 51), (1, 64, 27, 51), (1, 2, 67, 16)])
def test_ragged_shapes_match_the_restatement(cuda, B, S, T, J):
    from skeletondiffusion_amd import metrics as M

    tile = _lib.lib().sd_realism_frame_tile(J)
    assert T % tile != 0 and T > tile
    pred, target, limbseq, ref = _restated(B, S, T, J, 700 + J + S)
    p, g = pred.to(cuda), target.to(cuda)
    keys = expected_keys(T)
    _check(f"{(B, S, T, J)}", _single(M, p, g, limbseq, keys), ref)
    _check(f"{(B, S, T, J)} fused", _fused(M.limb_stats(p, limbseq, g), keys), ref)


def test_one_limb(cuda):
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, ref = _restated(2, 3, 33, 16, 731, L=1)
    assert len(limbseq) == 1
    keys = expected_keys(33)
    _check("one limb", _single(M, pred.to(cuda), target.to(cuda), limbseq, keys), ref)


def test_unaligned_base_gives_the_same_bits(cuda):
    """pred at 4, 8 and 12 bytes past a 16-byte boundary (the float-by-float head and tail of the staging) gives
    the bits of the aligned call."""
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, ref = _restated(2, 3, 33, 16, 741)
    g = target.to(cuda)
    aligned = M.limb_stats(pred.to(cuda), limbseq, g)
    _check("aligned", _fused(aligned, expected_keys(33)), ref)
    for off in (1, 2, 3):
        buf = torch.empty(pred.numel() + off, device=cuda)
        p = buf[off:].view(pred.shape)
        p.copy_(pred)
        assert p.data_ptr() % 16 == 4 * off
        r = M.limb_stats(p, limbseq, g)
        for name, a, b in zip(r._fields, r, aligned):
            assert _same_bits(a, b), (off, name)


def test_no_sequences(cuda):
    from skeletondiffusion_amd import metrics as M

    limbseq = _limbseq(16)
    L = len(limbseq)
    p, g = torch.empty(0, 5, 7, 16, 3, device=cuda), torch.empty(0, 7, 16, 3, device=cuda)
    r = M.limb_stats(p, limbseq, g)
    assert r.variance_none.shape == (0, 5, L) and r.jitter_none.shape == (0, 5, 6, L) and r.error_mean.shape == (0,)
    assert M.limb_length_variance(p, limbseq).shape == (0,)
    assert M.limb_length_variation_difference_wrtGT(g, p, limbseq, mode="none").shape == (0, 5, 6, L)
    acc = M.MPJPEAccumulator(device=cuda)
    acc.update(p[:, 0], g)
    assert int(acc.count) == 0 and tuple(acc.sum.shape) == (7, 16) and not acc.sum.any()


def test_a_nan_coordinate_stays_with_its_limbs(cuda):
    """One NaN coordinate (sequence 1, sample 2, frame 5, joint 3) makes NaN exactly the limbs of that joint in that
    sample, exactly the two steps around that frame, and every maximum / minimum above them; the rest keeps its bits."""
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, _ = _restated(2, 3, 33, 16, 741)
    bad = pred.clone()
    bad[1, 2, 5, 3, 1] = float("nan")
    g = target.to(cuda)
    clean, r = M.limb_stats(pred.to(cuda), limbseq, g), M.limb_stats(bad.to(cuda), limbseq, g)
    hit = torch.tensor([3 in l for l in limbseq])
    assert hit.any() and not hit.all()
    limb_mask = torch.zeros(2, 3, len(limbseq), dtype=torch.bool)
    limb_mask[1, 2] = hit
    step_mask = torch.zeros(2, 3, 32, len(limbseq), dtype=torch.bool)
    step_mask[1, 2, 4:6] = hit
    sample_mask = limb_mask.any(-1)
    seq_mask = sample_mask.any(-1)
    for name, mask in (("variance_none", limb_mask), ("jitter_mean_limb", limb_mask), ("jitter_max_limb", limb_mask),
                       ("jitter_min_limb", limb_mask), ("error_limb", limb_mask), ("jitter_none", step_mask),
                       ("variance_max_persample", sample_mask), ("variance_min_persample", sample_mask),
                       ("variance_mean_persample", sample_mask), ("jitter_max_persample", sample_mask),
                       ("jitter_min_persample", sample_mask), ("error_persample", sample_mask), ("variance_max", seq_mask),
                       ("variance_min", seq_mask), ("jitter_max", seq_mask), ("jitter_min", seq_mask), ("jitter_mean", seq_mask),
                       ("error_max", seq_mask), ("error_min", seq_mask), ("error_mean", seq_mask)):
        a, b = getattr(r, name).cpu(), getattr(clean, name).cpu()
        assert torch.equal(torch.isnan(a), mask), name
        assert torch.equal(a[~mask], b[~mask]), name
    d = M.limb_length_variation_difference_wrtGT(g, bad.to(cuda), limbseq, mode="none").cpu()
    assert torch.equal(torch.isnan(d), step_mask)
    _close(d[~step_mask], R_limb(pred, target, limbseq)["wrtgt_none"][~step_mask])


# ---- streaming frame error ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames_case(R, S, T, J, seed):
    pred, target = N((R, S, T, J, 3), seed), N((R, T, J, 3), seed + 1)
    idx = R_best_idx(pred, target)
    return pred, target, idx, R_frame_error(pred, target, idx)


@pytest.mark.parametrize("R,S,T,J", [(1, 1, 1, 16), (5, 7, 2, 21), (33, 7, 31, 51), (33, 1, 61, 16), (5, 7, 61, 51),
                                     (1, 7, 31, 21), (33, 7, 1, 16), (5, 1, 2, 51)])
def test_frame_error_update(cuda, R, S, T, J):
    """The whole profile and the window [T - 1, T) of the sample sd_best_sample picks, in one call, against the
    restatement: rows 1 / 5 / 33, samples 1 / 7, frames 1 / 2 / 31 / 61, J = 16 / 21 / 51."""
    from skeletondiffusion_amd import metrics as M

    pred, target, idx_ref, ref = _frames_case(R, S, T, J, 800 + R + S + T + J)
    p, g = pred.to(cuda), target.to(cuda)
    idx = M.best_sample(p, g)[0]
    assert torch.equal(idx.cpu(), idx_ref)
    full, last = M.MPJPEAccumulator(keep_time_dim=False, keep_joint_dim=True, device=cuda), M.FDEAccumulator(device=cuda)
    for acc in (full, last):
        acc.update(p, g, idx=idx) if S > 1 else acc.update(p[:, 0], g)
        assert acc.sum.dtype == torch.float64 and acc.sum.device.type == "cuda" and int(acc.count) == R
    assert tuple(full.sum.shape) == (T, J) and tuple(last.sum.shape) == (1, J)
    _close(full.sum.cpu() / R, ref)
    _close(last.sum.cpu() / R, ref[-1:])
    assert torch.equal(last.sum, full.sum[-1:])  # the same rows in the same order
    _close(last.compute(), ref[-1].mean())
    table = M.MPJPEAccumulator(device=cuda)
    table.update(p, g, best=True)
    _close(table.compute(), R_table(ref.mean(-1)))


def test_frame_error_state_is_bitwise_independent_of_the_batching(cuda):
    """37 rows in one call, as 5 + 32 and as 37 single rows: equal bits (each (frame, joint) adds its rows in
    ascending order onto the value it holds), also from a base 4 bytes past a 16-byte boundary."""
    from skeletondiffusion_amd import metrics as M

    pred, target, idx_ref, ref = _frames_case(37, 3, 61, 16, 861)
    p, g, idx = pred.to(cuda), target.to(cuda), idx_ref.to(cuda)
    buf = torch.empty(pred.numel() + 1, device=cuda)
    shifted = buf[1:].view(pred.shape)
    shifted.copy_(pred)
    states = []
    for src, split in ((p, [37]), (p, [5, 32]), (p, [1] * 37), (shifted, [37]), (shifted, [32, 5])):
        acc, r0 = M.MPJPEAccumulator(device=cuda), 0
        for n in split:
            acc.update(src[r0:r0 + n], g[r0:r0 + n], idx=idx[r0:r0 + n])
            r0 += n
        assert int(acc.count) == 37
        states.append(acc.sum.clone())
    _close(states[0].cpu() / 37, ref)
    for s in states[1:]:
        assert torch.equal(s, states[0])


def test_frame_error_index_that_is_no_sample(cuda):
    """A row whose index is outside [0, samples) adds NaN to all its sums and reads nothing of pred; the call ends
    cleanly and the other rows' calls are untouched.  A NaN coordinate reaches only its own (frame, joint)."""
    from skeletondiffusion_amd import metrics as M

    pred, target, _, _ = _frames_case(5, 7, 31, 21, 871)
    p, g = pred.to(cuda), target.to(cuda)
    idx = torch.tensor([0, 7, 6, -1, 2 ** 40], device=cuda)
    ref = R_frame_error(pred, target, idx.cpu().clamp(-1, 7)) * 5  # the sums: all NaN
    acc = M.MPJPEAccumulator(device=cuda)
    acc.update(p, g, idx=idx)
    torch.cuda.synchronize()
    assert torch.isnan(acc.sum).all() and torch.isnan(ref).all() and int(acc.count) == 5
    for r in range(5):
        one = M.MPJPEAccumulator(device=cuda)
        one.update(p[r:r + 1], g[r:r + 1], idx=idx[r:r + 1])
        if r in (0, 2):
            _close(one.sum.cpu(), R_frame_error(pred[r:r + 1], target[r:r + 1], idx[r:r + 1].cpu()))
        else:
            assert torch.isnan(one.sum).all()
    good = torch.tensor([0, 1, 6, 3, 2], device=cuda)
    clean, dirty = M.MPJPEAccumulator(device=cuda), M.MPJPEAccumulator(device=cuda)
    clean.update(p, g, idx=good)
    bad_p, bad_g = p.clone(), g.clone()
    bad_p[2, 6, 4, 9, 0] = float("nan")
    bad_g[4, 30, 20, 2] = float("nan")
    dirty.update(bad_p, bad_g, idx=good)
    mask = torch.zeros(31, 21, dtype=torch.bool)
    mask[4, 9] = mask[30, 20] = True
    assert torch.equal(torch.isnan(dirty.sum).cpu(), mask)
    assert torch.equal(dirty.sum.cpu()[~mask], clean.sum.cpu()[~mask])


def test_accumulators_match_the_fixture_and_the_gathered_best_sample(cuda):
    """The long case in its three uneven batches on the device against the fixture; `best=True` (no gathered copy)
    equals accumulating `metrics.choose_best_sample`'s gathered tensor, bit for bit; merge and all dims."""
    from skeletondiffusion_amd import metrics as M

    z = golden("validation")
    pred, target = long_case()
    p, g = pred.to(cuda), target.to(cuda)
    got = {}

    def feed(acc, first_sample, **kw):
        r0 = 0
        for n in z["long_batches"].tolist():
            acc.update(p[r0:r0 + n, 0] if first_sample else p[r0:r0 + n], g[r0:r0 + n], **kw)
            r0 += n
        return acc

    got["long_mpjpe_table"] = feed(M.MPJPEAccumulator(device=cuda), True).compute()
    got["long_mpjpe_joint_table"] = feed(M.MPJPEAccumulator(keep_joint_dim=True, device=cuda), True).compute()
    got["long_mpjpe_mean"] = feed(M.MPJPEAccumulator(keep_time_dim=False, device=cuda), True).compute()
    got["long_mpjpe_joint_mean"] = feed(M.MPJPEAccumulator(False, True, device=cuda), True).compute()
    got["long_fde"] = feed(M.FDEAccumulator(device=cuda), True).compute()
    best = feed(M.MPJPEAccumulator(device=cuda), False, best=True)
    got["long_best_mpjpe_table"] = best.compute()
    got["long_best_fde"] = feed(M.FDEAccumulator(device=cuda), False, best=True).compute()
    assert sorted(got) == sorted(LONG_KEYS)
    for k in LONG_KEYS:
        _close(got[k], z[k])
        _close(got[k], R_long(pred, target)[k])
    gathered = M.MPJPEAccumulator(device=cuda)
    r0 = 0
    for n in z["long_batches"].tolist():
        chosen, y = M.choose_best_sample(p[r0:r0 + n], g[r0:r0 + n])
        gathered.update(chosen, y)
        r0 += n
    assert torch.equal(gathered.sum, best.sum) and int(gathered.count) == int(best.count) == 11
    a, b = M.MPJPEAccumulator(device=cuda), M.MPJPEAccumulator(device="cpu")
    a.update(p[:5, 0], g[:5])
    b.update(pred[5:, 0], target[5:])
    _close(a.merge(b).compute(), z["long_mpjpe_table"])
    with pytest.raises(_lib.SkelDiffError):
        M.MPJPEAccumulator(device=cuda).update(pred, target, best=True)  # host tensors into a device state


# ---- the validation table --------------------------------------------------------------------------------------------
def _l1(a, b):
    return (a - b).abs().mean()


def test_validation_set_autoencoder(cuda):
    from skeletondiffusion_amd import evaluation as E

    pred, target = N((9, 61, 16, 3), 881), N((9, 61, 16, 3), 882)
    vs = E.validation_set("autoencoder", "h36m16", loss_fn=_l1, device=cuda)
    for lo, hi in ((0, 6), (6, 9)):
        vs.update(pred=pred[lo:hi].to(cuda), target=target[lo:hi].to(cuda), pred_input=0.5 * pred[lo:hi].to(cuda),
                  target_input=0.5 * target[lo:hi].to(cuda))
    out = vs.compute()
    assert list(out) == ["MPJPE", "MPJPE_AVG", "ADE", "FDE", "Loss"]
    prof = R_frame_error(pred[:, None], target)
    d = (pred.double() - target.double())
    ref = {"MPJPE": R_table(prof.mean(-1)), "MPJPE_AVG": R_table(prof.mean(-1)).mean(0),
           "ADE": d.flatten(2).norm(dim=-1).mean(-1).mean(), "FDE": prof[-1].mean(),
           "Loss": (6 * _l1(0.5 * pred[:6].double(), 0.5 * target[:6].double()) +
                    3 * _l1(0.5 * pred[6:].double(), 0.5 * target[6:].double())) / 9}
    assert out["MPJPE"].shape == (3,)
    for k, v in ref.items():
        _close(torch.as_tensor(out[k]), v)
    with pytest.raises(ValueError, match="pred_input"):
        vs.update(pred=pred[:2].to(cuda), target=target[:2].to(cuda))


def test_validation_set_diffusion(cuda):
    from skeletondiffusion_amd import evaluation as E

    pred, target = N((7, 5, 61, 16, 3), 891), N((7, 61, 16, 3), 892)
    limbseq = _limbseq(16)
    vs = E.validation_set("diffusion", "h36m16", loss_fn=_l1, device=cuda)
    plain = E.validation_set("diffusion", "h36m16", device=cuda)
    for lo, hi in ((0, 2), (2, 7)):
        p, g = pred[lo:hi].to(cuda), target[lo:hi].to(cuda)
        vs.update(pred=p, target=g, pred_input=0.5 * p, target_input=0.5 * g)
        plain.update(pred=p, target=g)
    out = vs.compute()
    assert list(out) == ["MPJPE", "MPJPE_AVG", "APD", "ADE", "LLVar", "Loss"]
    assert list(plain.compute()) == ["MPJPE", "MPJPE_AVG", "APD", "ADE", "LLVar"]
    p64, g64 = pred.double(), target.double()
    idx = R_best_idx(pred, target)
    prof = R_frame_error(pred, target, idx)
    best_in = 0.5 * p64[torch.arange(7), idx]
    flat = p64.flatten(2)
    ref = {"MPJPE": R_table(prof.mean(-1)), "MPJPE_AVG": R_table(prof.mean(-1)).mean(0),
           "APD": torch.stack([torch.pdist(x).mean() for x in flat]).mean(),
           "ADE": (p64 - g64[:, None]).flatten(3).norm(dim=-1).mean(-1).min(-1).values.mean(),
           "LLVar": R_limb(pred, target, limbseq)["variance_mean"].mean(),
           "Loss": (2 * _l1(best_in[:2], 0.5 * g64[:2]) + 5 * _l1(best_in[2:], 0.5 * g64[2:])) / 7}
    for k, v in ref.items():
        _close(torch.as_tensor(out[k]), v)
