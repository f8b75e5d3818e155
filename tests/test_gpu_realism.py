"""On-device body-realism, limb-angle and motion-profile metrics (skeletondiffusion_amd.metrics.realism and
the single functions built on it; C entries sd_realism_target / sd_realism) against
tests/golden/realism.npz -- the reference's own functions run in float64 -- and against the float64
restatement of tests/test_metrics_realism.py on the CPU.

Tolerance: that file's, |a - b| <= 1e-5 |b| + 1e-6, the relative term alone on the near-rigid case; NaN
patterns equal.  The device forms limb lengths, cosines, angles and every sum in float64 and rounds the
results to float32 (6e-8), the motion profile's joint steps are float32 norms (2e-7): both are far inside
the bound, so it is not widened for any shape here."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import _lib, synthetic
from test_metrics_realism import KEYS, R_all, R_mae, R_motion, R_smean_obs, _atol, _cases, _close, _edge_cases, _tables

pytestmark = pytest.mark.gpu
FIXTURE_CASES = ["normal", "rigid", "amass21", "mano51", "freeman17", "T2", "T1"]
SKEL_BY_J = {16: "h36m16", 21: "amass21", 17: "freeman17", 51: "mano51"}


def N(shape, seed, scale=1.0):
    return torch.from_numpy(synthetic.normal(shape, seed=seed)) * scale


def _tables_for(skel):
    from skeletondiffusion_amd import skeletons

    return skeletons.limbseq(skel), skeletons.limb_angles_idx(skel)


def _report(tag, got, ref):
    a, b = np.asarray(got.detach().cpu(), dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = ~np.isnan(b) & (b != 0)
    rel = float(np.max(np.abs(a - b)[ok] / np.abs(b)[ok])) if ok.any() else 0.0
    print(f"{tag}: max relative error {rel:.3e}")


def _check_all(tag, r, ref, atol=1e-6):
    """Every key of KEYS of a `Realism` against a dict of references."""
    for k in KEYS:
        _report(f"{tag} {k}", getattr(r, k), ref[k])
        _close(getattr(r, k), ref[k], atol)


@functools.lru_cache(maxsize=None)
def _restated(B, S, T, J, seed, scale=1.0):
    """Seeded inputs of a shape with its skeleton's tables and the float64 restatement, computed once."""
    limbseq, chains = _tables_for(SKEL_BY_J[J])
    pred, target = N((B, S, T, J, 3), seed, scale), N((B, T, J, 3), seed + 1, scale)
    ref = R_all(pred, target, limbseq, chains)
    ref["mae_persample"] = R_mae(target, pred, limbseq, chains, per_sample=True)
    return pred, target, limbseq, chains, ref


# ---- the fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_case(cuda, name):
    """Every function x mode x reduction, mae with and without if_return_cossim and the motion profile of
    the seven fixture cases, from the fused call and from the reference-signature functions."""
    from skeletondiffusion_amd import metrics as M

    z = golden("realism")
    skel, pred, target = {**_cases(), **_edge_cases()}[name]
    limbseq, chains = _tables(z, skel)
    p, g = pred.to(cuda), target.to(cuda)
    ref = {k: z[f"{name}_{k}"] for k in KEYS}
    _check_all(name, M.realism(p, g, limbseq, chains), ref, _atol(name))
    single = {}
    for red in ("mean", "persample", "none"):
        for mode in ("std", "var"):
            single[f"srmse_{mode}_{red}"] = M.limb_stretching_normed_rmse(p, g, limbseq, mode=mode, reduction=red)
            single[f"jrmse_{mode}_{red}"] = M.limb_jitter_normed_rmse(p, g, limbseq, mode=mode, reduction=red)
        single[f"smean_{red}"] = M.limb_stretching_normed_mean(p, g, limbseq, reduction=red)
        single[f"jmean_{red}"] = M.limb_jitter_normed_mean(p, g, limbseq, reduction=red)
    single["mae"] = M.mae(g, p, limbseq, chains)
    single["mae_cossim"] = M.mae(g, p, limbseq, chains, if_return_cossim=True)
    single["motion"] = M.motion_for_cmd(p)
    assert sorted(single) == sorted(KEYS)
    for k in KEYS:
        _close(single[k], ref[k], _atol(name))
    if name == "T1":
        assert single["motion"].shape == (2, 0) and bool(torch.isnan(single["jmean_none"]).all())


def test_fixture_slices_observation_target_and_stats_funcs(cuda):
    from skeletondiffusion_amd import evaluation as E, metrics as M

    z = golden("realism")
    _, pred, target = _cases()["normal"]
    limbseq, chains = _tables(z, "h36m16")
    p, g = pred.to(cuda), target.to(cuda)
    _close(M.mae(g, p, limbseq, chains, 5, 15), z["normal_mae_t5_15"])
    _close(M.mae(g, p, limbseq, chains, t0=5, t=15, if_return_cossim=True), z["normal_mae_cossim_t5_15"])
    per = M.mae(g, p, limbseq, chains, reduction="none")
    assert per.shape == (2, 7)
    _close(per, R_mae(target, pred, limbseq, chains, per_sample=True))
    obs = N((2, 10, 16, 3), 62).to(cuda)
    for red in ("mean", "persample", "none"):
        _close(M.limb_stretching_normed_mean(p, obs, limbseq, reduction=red, obs_as_target=True), z[f"normal_smean_obs_{red}"])
    with pytest.raises(ValueError):
        M.limb_stretching_normed_mean(p, obs, limbseq)  # body_realism.py:136
    with pytest.raises(_lib.SkelDiffError):  # angles against a target of another frame count
        M._realism(p, obs, limbseq, chains, {"angle"}, obs_as_target=True)
    funcs = E.get_stats_funcs("probabilistic", "h36m16")
    for name, key in (("StretchMean", "smean_mean"), ("JitterMean", "jmean_mean"), ("StretchRMSE", "srmse_std_mean"),
                      ("JitterRMSE", "jrmse_std_mean")):
        _close(funcs[name](pred=p, target=g, mm_gt=None), 100 * z[f"normal_{key}"], 1e-4)
    _close(funcs["MAE"](pred=p, target=g, mm_gt=None), z["normal_mae"])


# ---- one launch sequence, fixed order ----------------------------------------------------------------
def _fields(r):
    return {k: v for k, v in r._asdict().items() if v is not None}


def _bitwise(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


@pytest.mark.parametrize("angles", [True, False])
def test_fused_call_is_bitwise_the_single_functions(cuda, angles):
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, chains, _ = _restated(2, 5, 33, 21, 101)
    p, g = pred.to(cuda), target.to(cuda)
    r = M.realism(p, g, limbseq, chains if angles else None)
    for red in ("mean", "persample", "none"):
        for mode in ("std", "var"):
            assert _bitwise(getattr(r, f"srmse_{mode}_{red}"), M.limb_stretching_normed_rmse(p, g, limbseq, mode, red))
            assert _bitwise(getattr(r, f"jrmse_{mode}_{red}"), M.limb_jitter_normed_rmse(p, g, limbseq, mode, red))
        assert _bitwise(getattr(r, f"smean_{red}"), M.limb_stretching_normed_mean(p, g, limbseq, red))
        assert _bitwise(getattr(r, f"jmean_{red}"), M.limb_jitter_normed_mean(p, g, limbseq, red))
    assert _bitwise(r.motion, M.motion_for_cmd(p))
    if angles:
        assert _bitwise(r.mae, M.mae(g, p, limbseq, chains))
        assert _bitwise(r.mae_persample, M.mae(g, p, limbseq, chains, reduction="none"))
        assert _bitwise(r.mae_cossim, M.mae(g, p, limbseq, chains, if_return_cossim=True))
        assert _bitwise(r.mae_cossim_persample, M.mae(g, p, limbseq, chains, if_return_cossim=True, reduction="none"))
    else:
        assert r.mae is None and r.mae_persample is None and r.mae_cossim is None and r.mae_cossim_persample is None


def test_determinism_permutation_and_alignment(cuda):
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, chains, _ = _restated(2, 5, 33, 21, 101)
    p, g = pred.to(cuda), target.to(cuda)
    first = _fields(M.realism(p, g, limbseq, chains))
    for k, v in _fields(M.realism(p, g, limbseq, chains)).items():  # the same call again
        assert _bitwise(v, first[k]), k
    # permuting the samples permutes the per-sample and per-limb outputs bitwise
    perm = torch.tensor([3, 0, 4, 2, 1], device=cuda)
    q = _fields(M.realism(p[:, perm].contiguous(), g, limbseq, chains))
    for k, v in q.items():
        if k.endswith("_persample") or k.endswith("_none"):
            assert _bitwise(v, first[k][:, perm]), k
    # two samples with the same bytes give the same bits
    twin = p.clone()
    twin[:, 4] = twin[:, 1]
    t = _fields(M.realism(twin, g, limbseq, chains))
    for k, v in t.items():
        if k.endswith("_persample") or k.endswith("_none"):
            assert _bitwise(v[:, 4], v[:, 1]), k
    # pred 1, 2 or 3 floats past a 16-byte boundary (a view into a larger buffer)
    for shift in (1, 2, 3):
        big = torch.empty(p.numel() + 8, device=cuda)
        view = big[shift:shift + p.numel()].view(p.shape)
        view.copy_(p)
        assert view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        for k, v in _fields(M.realism(view, g, limbseq, chains)).items():
            assert _bitwise(v, first[k]), (shift, k)


# ---- frame tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [16, 51])
def test_frame_tile_boundaries(cuda, J):
    """T around the number of frames the prediction pass stages at a time (sd_realism_frame_tile)."""
    from skeletondiffusion_amd import metrics as M

    tile = _lib.lib().sd_realism_frame_tile(J)
    assert tile == {16: 32, 51: 13}[J]
    for T in (tile - 1, tile, tile + 1, 2 * tile + 1):
        pred, target, limbseq, chains, ref = _restated(1, 2, T, J, 200 + T)
        _check_all(f"J={J} T={T}", M.realism(pred.to(cuda), target.to(cuda), limbseq, chains), ref)


# ---- limits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 64, 5, 16), (2, 1, 7, 17)])
def test_sample_count_limits(cuda, shape):
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, chains, ref = _restated(*shape, 301)
    r = M.realism(pred.to(cuda), target.to(cuda), limbseq, chains)
    _check_all(f"S={shape[1]}", r, ref)
    _close(r.mae_persample, ref["mae_persample"])


def test_table_limits_64_joints_limbs_and_pairs(cuda):
    from skeletondiffusion_amd import metrics as M

    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.integers(0, 64, 64)
    limbseq = np.stack([a, (a + rng.integers(1, 64, 64)) % 64], 1).tolist()  # 64 limbs, two distinct joints each
    limbseq[0], limbseq[1] = [63, 0], [0, 63]
    pa = rng.integers(0, 64, 64)
    chains = [[int(x), int(y)] for x, y in zip(pa, (pa + rng.integers(1, 64, 64)) % 64)]  # 64 pairs
    chains[0] = [63, 0]
    T = 2 * _lib.lib().sd_realism_frame_tile(64) + 1
    pred, target = N((2, 3, T, 64, 3), 401), N((2, T, 64, 3), 402)
    _check_all("J=L=P=64", M.realism(pred.to(cuda), target.to(cuda), limbseq, chains), R_all(pred, target, limbseq, chains))


def test_coincident_joints_hit_the_denominator_clamp(cuda):
    """A limb of an angle pair with both joints at one point in pred: |a||b| = 0 is clamped to 1e-7
    (multimodal.py:80), the cosine is 0 and the angle 90 degrees, not NaN."""
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, chains, _ = _restated(2, 5, 33, 21, 101)
    pred = pred.clone()
    l = chains[0][1]  # a limb of the first chain's first pair
    pred[:, 1, :, limbseq[l][0]] = pred[:, 1, :, limbseq[l][1]]
    p, g = pred.to(cuda), target.to(cuda)
    for cossim in (False, True):
        got = M.mae(g, p, limbseq, chains, if_return_cossim=cossim, reduction="none")
        assert not bool(torch.isnan(got).any())
        _close(got, R_mae(target, pred, limbseq, chains, cossim=cossim, per_sample=True))
        _close(M.mae(g, p, limbseq, chains, if_return_cossim=cossim), R_mae(target, pred, limbseq, chains, cossim=cossim))


# ---- the evaluation's frame and joint counts -----------------------------------------------------------
def test_evaluation_shape_small_batch(cuda):
    """8 x 50 x 120 x 21 x 3 (12.9 MB): the release evaluation's samples, frames and joints."""
    from skeletondiffusion_amd import metrics as M

    pred, target, limbseq, chains, ref = _restated(8, 50, 120, 21, 501, 0.3)
    r = M.realism(pred.to(cuda), target.to(cuda), limbseq, chains)
    _check_all("8x50x120x21", r, ref)
    _close(r.mae_persample, ref["mae_persample"])
    _close(M.motion_for_cmd(pred.to(cuda)), R_motion(pred))
