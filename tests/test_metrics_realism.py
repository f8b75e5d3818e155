"""The reference's body-realism (limb stretching / jitter, src/metrics/body_realism.py:109-199),
limb-angle MAE (multimodal.py:76-102) and CMD (cmd.py:10-12, multimodal.py:10-13) metrics:
tests/golden/realism.npz (made by gen_golden_realism.py from the reference's own functions) against
a float64 restatement kept here, and `skeletondiffusion_amd.metrics.cmd`.  CPU only: the fixture
and the restatement are what on-device versions of these metrics are to be compared against.

Tolerance: the project's metric tolerance of tests/test_metrics.py, |a - b| <= 1e-5 |b| + 1e-6; on
the near-rigid case the relative term alone (its values go down to 1e-4, where the absolute floor
would hide a one-pass-variance bug).  The fixture holds the reference run in float64 on the float32
inputs: in float32 the reference's own StretchMean with reduction 'none' is off by up to 5e-2 of
its value on the near-rigid case (a difference of nearly equal lengths; gen_golden_realism.py prints
it), so no float32 run of it could be pinned at 1e-5."""
import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import synthetic

RTOL = 1e-5
REDUCTIONS = ("mean", "persample", "none")
KEYS = [f"{m}_{red}" for m in ("srmse_std", "srmse_var", "jrmse_std", "jrmse_var", "smean", "jmean")
        for red in REDUCTIONS] + ["mae", "mae_cossim", "motion"]


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


def _cases():
    """gen_golden_realism.py:cases, restated: name -> (skeleton, pred, target)."""
    rest = N((2, 1, 1, 16, 3), 53) * 0.3
    return {
        "normal": ("h36m16", N((2, 7, 20, 16, 3), 51), N((2, 20, 16, 3), 52)),
        "rigid": ("h36m16", rest + 1e-2 * N((2, 7, 20, 16, 3), 54), rest[:, 0] + 1e-3 * N((2, 20, 16, 3), 55)),
        "amass21": ("amass21", N((2, 5, 33, 21, 3), 56), N((2, 33, 21, 3), 57)),
        "mano51": ("mano51", N((1, 3, 4, 51, 3), 58), N((1, 4, 51, 3), 59)),
        "freeman17": ("freeman17", N((1, 2, 5, 17, 3), 60), N((1, 5, 17, 3), 61)),
    }


def _edge_cases():
    _, pred, target = _cases()["normal"]
    return {"T2": ("h36m16", pred[:, :, :2], target[:, :2]), "T1": ("h36m16", pred[:, :, :1], target[:, :1])}


def _tables(z, skel):
    """(limbseq as a list of pairs, limb_angles_idx as chains) of a skeleton, from the fixture."""
    limbseq = z[f"{skel}_limbseq"].tolist()
    pairs, chains, k = z[f"{skel}_angle_pairs"], [], 0
    for n in z[f"{skel}_chain_lengths"]:
        chains.append([int(pairs[k, 0])] + [int(p[1]) for p in pairs[k:k + n - 1]])
        k += n - 1
    return limbseq, chains


def _close(a, b, atol=1e-6):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    err = np.abs(a - b)[ok]
    assert np.all(err <= RTOL * np.abs(b)[ok] + atol), (float(err.max()), a, b)


def _atol(case):
    return 0.0 if case == "rigid" else 1e-6


# ---- float64 restatement ---------------------------------------------------------------------------
def _limb_len(x, limbseq):
    ls = torch.as_tensor(limbseq)
    return (x[..., ls[:, 0], :] - x[..., ls[:, 1], :]).norm(dim=-1)


def _reduce(v, reduction):
    return v.flatten(1).mean(-1) if reduction == "mean" else v.mean(-1) if reduction == "persample" else v


def R_all(pred, target, limbseq, chains):
    """Every quantity of the fixture (keys as gen_golden_realism.py:all_metrics) in float64.
    Deviations are taken from the ground truth's mean length directly, never as E[x^2] - mean^2."""
    pred, target = pred.double(), target.double()
    ll = _limb_len(pred, limbseq)                           # (B, S, T, L)
    gt = _limb_len(target, limbseq).mean(-2)[:, None]       # (B, 1, L)
    dev2 = ((ll - gt[:, :, None]) ** 2).mean(-2)
    jit = (ll[:, :, 1:] - ll[:, :, :-1]).abs()
    out = {}
    for red in REDUCTIONS:
        out[f"srmse_std_{red}"] = _reduce(dev2.sqrt() / gt, red)
        out[f"srmse_var_{red}"] = _reduce(dev2 / gt, red)
        out[f"jrmse_std_{red}"] = _reduce((jit ** 2).mean(-2).sqrt() / gt, red)
        out[f"jrmse_var_{red}"] = _reduce((jit ** 2).mean(-2) / gt, red)
        out[f"smean_{red}"] = _reduce((ll.mean(-2) - gt).abs() / gt, red)
        out[f"jmean_{red}"] = _reduce(jit.mean(-2) / gt, red)
    out["mae"] = R_mae(target, pred, limbseq, chains)
    out["mae_cossim"] = R_mae(target, pred, limbseq, chains, cossim=True)
    out["motion"] = R_motion(pred)
    return out


def R_smean_obs(pred, obs, limbseq, red):
    gt = _limb_len(obs.double(), limbseq).mean(-2)[:, None]
    return _reduce((_limb_len(pred.double(), limbseq).mean(-2) - gt).abs() / gt, red)


def R_mae(target, pred, limbseq, chains, t0=0, t=-1, cossim=False, per_sample=False):
    target, pred = target.double(), pred.double()
    end = pred.shape[2] if t == -1 else t
    pred, target = pred[:, :, t0:end], target[:, t0:end]
    ls = torch.as_tensor(limbseq).sort(dim=-1)[0]
    ap = torch.tensor([[c[i], c[i + 1]] for c in chains for i in range(len(c) - 1)])

    def cos(x):
        v = x[..., ls[:, 1], :] - x[..., ls[:, 0], :]
        a, b = v[..., ap[:, 0], :], v[..., ap[:, 1], :]
        den = (a.norm(dim=-1) * b.norm(dim=-1)).clamp_min(1e-7)
        return (a * b).sum(-1) / den

    cp, cg = cos(pred), cos(target)[:, None]
    diff = cp - cg if cossim else torch.acos(cp.clamp(-1, 1)) - torch.acos(cg.clamp(-1, 1))
    per = diff.abs().mean(-1).mean(-1) * (180 / np.pi)
    return per if per_sample else per.min(-1).values


def R_motion(pred):
    pred = pred.double()
    return (pred[:, :, 1:] - pred[:, :, :-1]).norm(dim=-1).mean(1).mean(-1)


# ---- tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["normal", "rigid", "amass21", "mano51", "freeman17", "T2", "T1"])
def test_restatement_reproduces_reference(name):
    """Every function x mode x reduction, mae with and without if_return_cossim and the motion
    profile: J = 16 ("normal" and near-rigid), J = 21 (T = 33, S = 5), J = 51, J = 17, and the
    T = 2 / T = 1 edges (NaN jitter and an empty motion profile, as the reference gives)."""
    z = golden("realism")
    skel, pred, target = {**_cases(), **_edge_cases()}[name]
    limbseq, chains = _tables(z, skel)
    got = R_all(pred, target, limbseq, chains)
    assert sorted(got) == sorted(KEYS)  # every quantity is compared, none skipped
    for k in KEYS:
        _close(got[k], z[f"{name}_{k}"], _atol(name))
    if name == "T1":
        assert np.isnan(z["T1_jmean_mean"]).all() and np.isnan(z["T1_jrmse_std_none"]).all()
        assert z["T1_motion"].shape == (2, 0)


def test_one_pass_variance_misses_the_rigid_case():
    """The near-rigid case does what it is there for: float32 E[x^2] - mean^2 taken around zero
    instead of the deviation from the ground truth's mean misses the relative tolerance."""
    z = golden("realism")
    skel, pred, target = _cases()["rigid"]
    limbseq, _ = _tables(z, skel)
    ll = _limb_len(pred, limbseq)  # float32
    gt = _limb_len(target, limbseq).mean(-2)[:, None]
    one_pass = (ll ** 2).mean(-2) - 2 * gt * ll.mean(-2) + gt ** 2
    ref = z["rigid_srmse_var_none"]
    err = np.abs((one_pass / gt).double().numpy() - ref) / np.abs(ref)
    assert err.max() > RTOL


def test_restatement_slices_and_observation_target():
    z = golden("realism")
    _, pred, target = _cases()["normal"]
    limbseq, chains = _tables(z, "h36m16")
    _close(R_mae(target, pred, limbseq, chains, 5, 15), z["normal_mae_t5_15"])
    _close(R_mae(target, pred, limbseq, chains, 5, 15, cossim=True), z["normal_mae_cossim_t5_15"])
    assert R_mae(target, pred, limbseq, chains, per_sample=True).shape == (2, 7)
    obs = N((2, 10, 16, 3), 62)
    for red in REDUCTIONS:
        _close(R_smean_obs(pred, obs, limbseq, red), z[f"normal_smean_obs_{red}"])


def test_limb_tables_of_the_fixture():
    """The reference's limb tables: in range, within the 64-pair limit, and the same limbs as the
    package's own skeleton graphs (skeletondiffusion_amd.skeletons)."""
    from skeletondiffusion_amd.skeletons import skeleton

    z = golden("realism")
    for skel, J in (("h36m16", 16), ("amass21", 21), ("freeman17", 17), ("mano51", 51)):
        limbseq, chains = _tables(z, skel)
        assert 0 <= min(map(min, limbseq)) and max(map(max, limbseq)) < J and len(limbseq) <= 64
        assert max(map(max, chains)) < len(limbseq)
        assert sum(len(c) - 1 for c in chains) == len(z[f"{skel}_angle_pairs"]) <= 64
        _, node_limbs, _, _ = skeleton(skel)
        assert sorted(tuple(sorted(l)) for l in limbseq) == sorted(tuple(sorted(l)) for l in node_limbs)


def test_cmd_matches_reference():
    from skeletondiffusion_amd import metrics as M

    z = golden("realism")
    profile = z["normal_motion"].mean(0)
    _close(M.cmd(profile, float(z["cmd_ref"])), z["cmd_value"])
    _close(M.cmd(torch.from_numpy(profile), float(z["cmd_ref"])), z["cmd_value"])
    _close(M.cmd(profile.tolist(), float(z["cmd_ref"])), z["cmd_value"])
    assert M.cmd(np.zeros(0), 1.0) == 0.0
    assert "cmd" in M.__all__
