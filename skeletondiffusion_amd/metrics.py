"""On-device evaluation metrics with the reference's signatures (src/metrics/multimodal.py),
computed by libskeldiff (sd_pairwise_distances / sd_ade_fde) where the sampled latents or the
decoded motions already live.  Inputs must be ROCm tensors (no CPU path); results are float32
tensors on the same device, one value per sequence (or per (sequence, sample) for
reduction != 'mean'), reduced in a fixed order (deterministic).

    lat_apd(lat_pred)                 multimodal.py:137-151  mean pairwise L1 over samples
    apd(pred, t0=0, t=-1)             multimodal.py:15-35    mean pairwise L2 over samples
    ade(target, pred, t0, t, reduction)  multimodal.py:44-57  min over samples of mean-frame L2
    fde(target, pred, t0, t, reduction)  multimodal.py:60-73  min over samples of last-frame L2
    mpjpe(target, pred)               multimodal.py:37-42    min over samples of the mean per-joint L2
    choose_best_sample / get_best_sample_idx(out, y)  metrics/utils.py:12-30  the sample closest to y
    best_sample(out, y, tail)         eval_utils.py:59-62    index, distance, trajectory and its last
                                      `tail` frames in one launch sequence (sd_best_sample)

    limb_stretching_normed_rmse / _mean, limb_jitter_normed_rmse / _mean(pred, target, limbseq, ...)
                                      body_realism.py:109-199  limb stretching and jitter over the gt limb length
    mae(target, pred, limbseq, limb_angles_idx, t0, t, if_return_cossim)  multimodal.py:76-102  limb-angle error
    motion_for_cmd(pred)              cmd.py:10-12           the CMD's motion profile (B, T - 1)
    realism(pred, target, limbseq, limb_angles_idx)  all of the four lines above from one read of pred
                                      (sd_realism_target + sd_realism; float64 inside)

    FIDClassifier(state_dict, device) fid_classifier.py:5-57  get_fid_features / features: the 2-layer GRU
                                      classifier's 30 activations per future, one persistent launch (sd_fid_features)
    FIDAccumulator(classifier)        fid.py:91-129          update / merge / all_reduce / reset / compute: float64
                                      (count, sum x, sum x x^T) on the device (sd_fid_stats_update)
    frechet_distance(mu1, s1, mu2, s2)  fid.py:17-68         host, float64, eigenvalues instead of scipy's sqrtm
    APDEAccumulator(gt_apd)           apde.py:9-48           update / merge / all_reduce / reset / compute: mean
                                      |APD(pred) - APD(multimodal gt)|; the table: multimodal_gt.MultimodalGT.gt_apd

    diverse_rank(pred, target, n, from_closest)  ranking.py:3-63  farthest-point greedy over each sequence's samples
                                      (sd_diverse_rank; up to 255 samples), with the reference's
    find_samples_maxapd_wrtGT(pred, target, num_chosen_samples) and get_closest_and_nfurthest_maxapd(y_pred, y_gt, n)
    CMDAccumulator(mean_motion_per_class)  cmd.py:15-57    class-wise CMD: float64 sums per class on the device
                                      (sd_class_sum), update / merge / all_reduce / reset / motion_per_class / compute
    MetricAccumulator(return_op)      metric_storer.py       mean / max / min of per-sequence values, float64 on the device

    limb_length_variance / limb_length_jitter(pred, limbseq, mode, if_per_sample), limb_length_error /
    limb_length_variation_difference_wrtGT(target, pred, limbseq, mode)   body_realism.py:4-107
    limb_stats(pred, limbseq, target)  all of them from one read of pred (sd_limb_stats)
    format_metric_time_table(profile)  metrics/utils.py:5-10  frames 0, 30, 60, ... of a per-frame profile
    MPJPEAccumulator / FDEAccumulator  ignite_mpjpe.py, ignite_fde.py  update / merge / all_reduce / reset / compute:
                                      float64 sums per (frame, joint) on the device (sd_frame_error_update); the
                                      best sample is read where it lies (`best=True` or `idx=`)

Up to 64 samples per sequence (the release evaluation draws 50); up to 64 joints, limbs and angle pairs.

cmd(val_per_frame, val_ref) (multimodal.py:10-13) is the one host-side function here: the CMD score of
a class's mean motion profile, a sum over at most a few hundred frame steps.
"""
from __future__ import annotations

import collections
import ctypes

import torch

from . import _lib
from ._lib import SkelDiffError, check


def _device_tensor(x: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.device.type != "cuda":
        raise SkelDiffError(f"{name}: metrics run on the MI355X HIP engine only; pass a ROCm tensor")
    return x.detach().to(torch.float32).contiguous()


def _time_slice(x: torch.Tensor, t0: int, t: int, axis: int) -> torch.Tensor:
    """multimodal.py:4-8: frames [t0, t) of `axis`, or [t0, end) for t == -1."""
    end = x.shape[axis] if t == -1 else t
    return x.narrow(axis, t0, end - t0)


def _flat(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _pairwise(x: torch.Tensor, want_l1: bool) -> torch.Tensor:
    B, S = x.shape[:2]
    x = _device_tensor(x.reshape(B, S, _flat(x.shape[2:])), "pairwise")
    out = torch.empty(B, device=x.device, dtype=torch.float32)
    l1 = out if want_l1 else None
    l2 = None if want_l1 else out
    stream = torch.cuda.current_stream(x.device).cuda_stream
    check(_lib.lib().sd_pairwise_distances(x.data_ptr(), B, S, x.shape[2], _lib.ptr(l1), _lib.ptr(l2), stream))
    return out


def lat_apd(lat_pred: torch.Tensor, **kwargs) -> torch.Tensor:
    """Average pairwise L1 distance between the samples in latent space; lat_pred
    (batch, num_samples, ...) -> (batch,)."""
    return _pairwise(lat_pred, True)


def apd(pred: torch.Tensor, t0: int = 0, t: int = -1, **kwargs) -> torch.Tensor:
    """Average pairwise L2 distance; pred (batch, num_samples, seq_length, ...) -> (batch,)."""
    pred = _time_slice(pred, t0, t, 2)
    B, S = pred.shape[:2]
    if S == 1:  # multimodal.py:19-20
        return torch.tensor([0] * B, device=pred.device)
    return _pairwise(pred, False)


def _ade_fde(target, pred, t0, t, reduction, want_ade):
    pred, target = _time_slice(pred, t0, t, 2), _time_slice(target, t0, t, 1)
    B, S, T = pred.shape[:3]
    p = _device_tensor(pred.reshape(B, S, T, _flat(pred.shape[3:])), "pred")
    g = _device_tensor(target.reshape(B, T, _flat(target.shape[2:])), "target")
    if g.shape[2] != p.shape[3]:
        raise ValueError(f"target frames have {g.shape[2]} features, pred frames {p.shape[3]}")
    dev = p.device
    best = torch.empty(B, device=dev, dtype=torch.float32)
    per = torch.empty(B, S, device=dev, dtype=torch.float32) if reduction != "mean" else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (best, None, per, None) if want_ade else (None, best, None, per)
    check(_lib.lib().sd_ade_fde(p.data_ptr(), g.data_ptr(), B, S, T, p.shape[3], *(_lib.ptr(a) for a in args), stream))
    return best if reduction == "mean" else per


def ade(target: torch.Tensor, pred: torch.Tensor, t0: int = 0, t: int = -1, reduction: str = "mean", **kwargs):
    """target (batch, seq_length, ...), pred (batch, num_samples, seq_length, ...): min over samples
    of the mean over frames of the L2 distance (reduction 'mean'), else the (batch, num_samples)
    distances.  The minimum is torch.min's, as the reference's `dist.min(axis=-1).values`: a sample
    with a NaN makes its sequence's value NaN; a sample with an Inf distance is passed over."""
    return _ade_fde(target, pred, t0, t, reduction, True)


def fde(target: torch.Tensor, pred: torch.Tensor, t0: int = 0, t: int = -1, reduction: str = "mean", **kwargs):
    """As ade, on the last frame of the slice only."""
    return _ade_fde(target, pred, t0, t, reduction, False)


def _mm(target, pred, mm_gt, t0, t, want_ade):
    pred = _time_slice(pred, t0, t, 2)
    B, S, T = pred.shape[:3]
    if len(mm_gt) != B:
        raise ValueError(f"mm_gt has {len(mm_gt)} entries for {B} sequences")
    p = _device_tensor(pred.reshape(B, S, T, _flat(pred.shape[3:])), "pred")
    dev, F = p.device, p.shape[3]
    counts = [int(g.shape[0]) for g in mm_gt]
    if min(counts, default=1) == 0:  # the reference's reshape of an empty set raises (multimodal.py:113)
        raise RuntimeError("mmade/mmfde: a sequence has no multimodal ground truths")
    parts = [_time_slice(_device_tensor(g, "mm_gt"), t0, t, 1).reshape(g.shape[0], T, -1) for g in mm_gt if g.shape[0]]
    for g in parts:
        if g.shape[2] != F:
            raise ValueError(f"mm_gt frames have {g.shape[2]} features, pred frames {F}")
    gts = torch.cat(parts).contiguous() if parts else torch.empty((0, T, F), device=dev)
    npairs = gts.shape[0]
    cnt = torch.tensor(counts, dtype=torch.int64)
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(cnt, 0)
    off = off.to(dev)
    pair_seq = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), cnt).to(dev)
    pair = torch.empty(max(npairs, 1), device=dev, dtype=torch.float32)
    out = torch.empty(B, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (pair, None, out, None) if want_ade else (None, pair, None, out)
    check(_lib.lib().sd_mm_ade_fde(p.data_ptr(), gts.data_ptr() if npairs else None, pair_seq.data_ptr() if npairs else None,
                                   npairs, off.data_ptr(), B, S, T, F, *(_lib.ptr(a) for a in args), stream))
    return out


def mmade(target: torch.Tensor, pred: torch.Tensor, mm_gt, t0: int = 0, t: int = -1, **kwargs) -> torch.Tensor:
    """Multimodal ADE (multimodal.py:108-120): pred (batch, num_samples, seq_length, ...), mm_gt a
    sequence of batch tensors (n_gts_i, seq_length, ...): per sequence the mean over its ground
    truths of the min over samples of the mean-over-frames L2 distance (RuntimeError for a
    sequence without ground truths, as the reference).  `target` is unused, as in the reference.
    As in ade, a sample with a NaN makes every minimum of its sequence, and so the sequence's mean, NaN."""
    return _mm(target, pred, mm_gt, t0, t, True)


def mmfde(target: torch.Tensor, pred: torch.Tensor, mm_gt, t0: int = 0, t: int = -1, **kwargs) -> torch.Tensor:
    """Multimodal FDE (multimodal.py:122-135): as mmade on the last frame of the slice."""
    return _mm(target, pred, mm_gt, t0, t, False)


def _best_sample(out, y, tail, want_dist, want_idx, want_best):
    """One sd_best_sample call: (per_sample (B, S), dist, idx, best, tail), the unwanted ones None."""
    p, g = _device_tensor(out, "pred"), _device_tensor(y, "target")
    if p.dim() != 5 or g.dim() != 4 or tuple(g.shape) != (p.shape[0],) + tuple(p.shape[2:]):
        raise ValueError(f"best sample: pred (B, S, T, J, 3) and target (B, T, J, 3) expected, got "
                         f"{tuple(p.shape)} and {tuple(g.shape)}")
    B, S, T, J, C = p.shape
    tail = 0 if tail is None else int(tail)
    dev = p.device
    per = torch.empty(B, S, device=dev, dtype=torch.float32)
    dist = torch.empty(B, device=dev, dtype=torch.float32) if want_dist else None
    idx = torch.empty(B, device=dev, dtype=torch.int64) if want_idx else None
    best = torch.empty(B, T, J, C, device=dev, dtype=torch.float32) if want_best else None
    # sd_best_sample checks 0 <= tail <= T before it reads the shape of tail_out
    last = torch.empty(B, tail, J, C, device=dev, dtype=torch.float32) if 0 < tail <= T else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(_lib.lib().sd_best_sample(p.data_ptr(), g.data_ptr(), B, S, T, J, C, tail, per.data_ptr(), _lib.ptr(dist),
                                    _lib.ptr(idx), _lib.ptr(best), _lib.ptr(last), stream))
    return per, dist, idx, best, last


def mpjpe(target: torch.Tensor, pred: torch.Tensor, reduction: str = "mean", **kwargs) -> torch.Tensor:
    """Mean per-joint position error (multimodal.py:37-42): target (batch, seq_length, joints, 3),
    pred (batch, num_samples, seq_length, joints, 3): min over samples of the mean over frames and
    joints of the per-joint L2 distance -> (batch,).  As ade / fde, another `reduction` returns the
    (batch, num_samples) distances before the minimum."""
    per, dist, _, _, _ = _best_sample(pred, target, None, reduction == "mean", False, False)
    return dist if reduction == "mean" else per


def best_sample(out: torch.Tensor, y: torch.Tensor, tail=None):
    """The sample closest to the ground truth and what the long-term rollout needs of it
    (eval_utils.py:59-62), in one launch sequence and without a host synchronisation: out
    (batch, num_samples, seq_length, joints, 3), y (batch, seq_length, joints, 3) ->
    (idx int64 (batch,), dist f32 (batch,), best (batch, seq_length, joints, 3),
    best[:, -tail:] (batch, tail, joints, 3) or None without `tail`).  idx is
    torch.min(dim).indices of the per-sample distances: the first minimum, the first NaN if any."""
    _, dist, idx, best, last = _best_sample(out, y, tail, True, True, True)
    return idx, dist, best, last


def get_best_sample_idx(out: torch.Tensor, y: torch.Tensor):
    """metrics/utils.py:22-30: (out[b, idx[b]] (batch, seq_length, joints, 3), the (batch,
    num_samples) bool one-hot of idx).  The mask stays on the device."""
    _, _, idx, best, _ = _best_sample(out, y, None, False, True, True)
    mask = idx.unsqueeze(1) == torch.arange(out.shape[1], device=idx.device).unsqueeze(0)
    return best, mask


def choose_best_sample(out: torch.Tensor, y: torch.Tensor):
    """metrics/utils.py:12-20: (the sample closest to y, y)."""
    _, _, _, best, _ = _best_sample(out, y, None, False, False, True)
    return best, y


def cmd(val_per_frame, val_ref) -> float:
    """Cumulative motion distribution of one class (multimodal.py:10-13): val_per_frame the class's
    mean motion profile M_t (frames - 1 values: array, list or tensor), val_ref its dataset mean
    motion M: sum_t (T - t) |M_t - M|.  The class-weighted aggregation over a dataset
    (src/metrics/cmd.py:15-31) is `CMDAccumulator`."""
    import numpy as np

    v = np.asarray(val_per_frame.detach().cpu() if torch.is_tensor(val_per_frame) else val_per_frame, dtype=np.float64)
    T = len(v) + 1
    return float(np.sum((T - np.arange(1, T)) * np.abs(v - float(val_ref))))


# ---- body realism, limb angles, motion profile (sd_realism_target + sd_realism) --------
_QUANTITIES = ("srmse_std", "srmse_var", "jrmse_std", "jrmse_var", "smean", "jmean")
_REDUCTIONS = ("mean", "persample", "none")
Realism = collections.namedtuple(
    "Realism", [f"{q}_{r}" for q in _QUANTITIES for r in _REDUCTIONS] +
    ["mae", "mae_persample", "mae_cossim", "mae_cossim_persample", "motion"])
Realism.__doc__ = """What `realism` returns: `{quantity}_{reduction}` for srmse / jrmse (`std`, `var`), smean and jmean
(limb_stretching_normed_rmse, limb_jitter_normed_rmse, limb_stretching_normed_mean, limb_jitter_normed_mean)
with reduction mean (B,), persample (B, S) and none (B, S, L); mae / mae_cossim (B,) and their (B, S)
values before the minimum (None without limb_angles_idx); motion (B, T - 1)."""


def _int_table(rows, name: str):
    """A (n, 2) integer table (list, array or tensor) as a host int32 ctypes array and n."""
    rows = rows.tolist() if hasattr(rows, "tolist") else list(rows)
    flat = []
    for r in rows:
        if len(r) != 2:
            raise ValueError(f"{name}: rows of two indices expected, got {r}")
        flat += [int(r[0]), int(r[1])]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat), len(rows)


def _angle_pairs(limb_angles_idx):
    """multimodal.py:87: the consecutive limb pairs of every kinematic chain."""
    return [[kin[i], kin[i + 1]] for kin in limb_angles_idx for i in range(len(kin) - 1)]


def _realism(pred, target, limbseq, limb_angles_idx, want, obs_as_target=False):
    """One sd_realism_target + sd_realism call computing the groups in `want` (a subset of 'none',
    'persample', 'mean', 'angle', 'cossim', 'motion'); -> dict of the raw output arrays."""
    p, g = _device_tensor(pred, "pred"), _device_tensor(target, "target")
    if p.dim() != 5 or g.dim() != 4 or p.shape[4] != 3 or (g.shape[0],) + tuple(g.shape[2:]) != (p.shape[0],) + tuple(p.shape[3:]):
        raise ValueError(f"realism: pred (B, S, T, J, 3) and target (B, T, J, 3) expected, got {tuple(p.shape)} and "
                         f"{tuple(g.shape)}")
    B, S, T, J, _ = p.shape
    Tt = g.shape[1]
    if Tt != T and not obs_as_target:  # body_realism.py:115
        raise ValueError(f"realism: target has {Tt} frames, pred {T} (only limb_stretching_normed_mean takes another "
                         "count, with obs_as_target)")
    angles = "angle" in want or "cossim" in want
    limbs, L = _int_table(limbseq, "limbseq")
    pairs, P = _int_table(_angle_pairs(limb_angles_idx) if angles else [], "limb_angles_idx")
    dev = p.device
    f32 = dict(device=dev, dtype=torch.float32)
    f64 = dict(device=dev, dtype=torch.float64)
    gt_len = torch.empty(B, L, **f64)
    gt_cos = torch.empty(B, Tt, P, **f64) if angles else None
    gt_ang = torch.empty(B, Tt, P, **f64) if "angle" in want else None
    o = {
        "none": torch.empty(6, B, S, L, **f32) if "none" in want else None,
        "persample": torch.empty(6, B, S, **f32) if "persample" in want else None,
        "scratch": torch.empty(6, B, S, L, **f64) if "mean" in want else None,
        "mean": torch.empty(6, B, **f32) if "mean" in want else None,
        "angle_ps": torch.empty(B, S, **f32) if "angle" in want else None,
        "cossim_ps": torch.empty(B, S, **f32) if "cossim" in want else None,
        "angle": torch.empty(B, **f32) if "angle" in want else None,
        "cossim": torch.empty(B, **f32) if "cossim" in want else None,
        "motion_scratch": torch.empty(B, S, T - 1, **f32) if "motion" in want else None,
        "motion": torch.empty(B, T - 1, **f32) if "motion" in want else None,
    }
    stream = torch.cuda.current_stream(dev).cuda_stream
    L_ = _lib.lib()
    check(L_.sd_realism_target(g.data_ptr(), B, Tt, J, limbs, L, pairs, P, gt_len.data_ptr(), _lib.ptr(gt_cos),
                               _lib.ptr(gt_ang), stream))
    check(L_.sd_realism(p.data_ptr(), B, S, T, J, limbs, L, pairs, P, gt_len.data_ptr(), _lib.ptr(gt_cos),
                        _lib.ptr(gt_ang), Tt, *(_lib.ptr(o[k]) for k in ("none", "persample", "scratch", "mean", "angle_ps",
                                                                        "cossim_ps", "angle", "cossim", "motion_scratch",
                                                                        "motion")), stream))
    return o


def realism(pred: torch.Tensor, target: torch.Tensor, limbseq, limb_angles_idx=None) -> Realism:
    """Every body-realism quantity, the limb-angle errors and the motion profile from one launch
    sequence and one read of pred (B, S, T, J, 3); target (B, T, J, 3); limbseq (L, 2) joint indices,
    limb_angles_idx the kinematic chains of limb indices (`skeletons.limbseq / limb_angles_idx`).
    Without limb_angles_idx the angle fields are None and no acos is evaluated.  -> `Realism`."""
    want = {"none", "persample", "mean", "motion"} | ({"angle", "cossim"} if limb_angles_idx is not None else set())
    o = _realism(pred, target, limbseq, limb_angles_idx, want)
    vals = [o[r][q] for q in range(6) for r in _REDUCTIONS]
    return Realism(*vals, o["angle"], o["angle_ps"], o["cossim"], o["cossim_ps"], o["motion"])


def _limb_metric(q, pred, target, limbseq, reduction, obs_as_target=False):
    r = reduction if reduction in ("mean", "persample") else "none"
    return _realism(pred, target, limbseq, None, {r}, obs_as_target)[r][q]


def _mode(mode):
    assert mode in ("std", "var"), f"Mode {mode} not supported"  # body_realism.py:110
    return 0 if mode == "std" else 1


def limb_stretching_normed_rmse(pred, target, limbseq, mode="std", reduction="mean", **kwargs):
    """body_realism.py:109-129: per limb sqrt (mode 'std') or not ('var') of the mean over frames of
    (length - gt mean length)^2, over the gt mean length; reduction 'mean' (B,), 'persample' (B, S), else (B, S, L)."""
    return _limb_metric(_mode(mode), pred, target, limbseq, reduction)


def limb_jitter_normed_rmse(pred, target, limbseq, mode="std", reduction="mean", **kwargs):
    """body_realism.py:150-176: as limb_stretching_normed_rmse on the frame-to-frame change of the limb lengths."""
    return _limb_metric(2 + _mode(mode), pred, target, limbseq, reduction)


def limb_stretching_normed_mean(pred, target, limbseq, reduction="mean", obs_as_target=False, **kwargs):
    """body_realism.py:131-147: |mean limb length - gt mean length| / gt mean length; with obs_as_target
    the target may have another frame count (the observation)."""
    return _limb_metric(4, pred, target, limbseq, reduction, obs_as_target)


def limb_jitter_normed_mean(pred, target, limbseq, reduction="mean", **kwargs):
    """body_realism.py:178-199: mean |frame-to-frame change of the limb length| / gt mean length."""
    return _limb_metric(5, pred, target, limbseq, reduction)


def mae(target, pred, limbseq, limb_angles_idx, t0=0, t=-1, if_return_cossim=False, reduction="mean", **kwargs):
    """Limb-angle error in degrees (multimodal.py:76-102): min over samples of the mean over frames and
    angle pairs of |acos(cos_pred) - acos(cos_gt)| (of |cos_pred - cos_gt| with if_return_cossim), times
    180 / pi.  As ade / mpjpe, another `reduction` returns the (batch, num_samples) values before the minimum."""
    pred, target = _time_slice(pred, t0, t, 2), _time_slice(target, t0, t, 1)
    k = "cossim" if if_return_cossim else "angle"
    o = _realism(pred, target, limbseq, limb_angles_idx, {k})
    return o[k] if reduction == "mean" else o[k + "_ps"]


def motion_for_cmd(pred: torch.Tensor) -> torch.Tensor:
    """cmd.py:10-12: pred (B, S, T, J, 3) -> (B, T - 1), the mean over samples and joints of the
    joints' frame-to-frame displacement."""
    p = _device_tensor(pred, "pred")
    if p.dim() != 5 or p.shape[4] != 3:
        raise ValueError(f"motion_for_cmd: pred (B, S, T, J, 3) expected, got {tuple(p.shape)}")
    B, S, T = p.shape[:3]
    limbs, _ = _int_table([[0, 0]], "limbseq")  # no limb output is asked for; the argument check wants one limb
    gt_len = torch.ones(B, 1, device=p.device, dtype=torch.float64)
    scratch = torch.empty(B, S, T - 1, device=p.device, dtype=torch.float32)
    motion = torch.empty(B, T - 1, device=p.device, dtype=torch.float32)
    stream = torch.cuda.current_stream(p.device).cuda_stream
    check(_lib.lib().sd_realism(p.data_ptr(), B, S, T, p.shape[3], limbs, 1, None, 0, gt_len.data_ptr(), None, None, T,
                                *([None] * 8), scratch.data_ptr(), motion.data_ptr(), stream))
    return motion


# ---- limb-length statistics of the validation pass (sd_limb_stats) ----------------------------------
_LIMB_MODES = ("mean", "max", "min", "none")
LimbStats = collections.namedtuple(
    "LimbStats", ["variance_none"] + [f"variance_{m}{r}" for m in _LIMB_MODES[:3] for r in ("_persample", "")] +
    ["jitter_none"] + [f"jitter_{m}{r}" for m in _LIMB_MODES[:3] for r in ("_limb", "_persample", "")] +
    ["error_limb", "error_persample", "error_mean", "error_max", "error_min"])
LimbStats.__doc__ = """What `limb_stats` returns.  variance_none (B, S, L) the unbiased variance of each limb's length over
the frames; jitter_none (B, S, T - 1, L) the frame-to-frame change |len_t - len_{t-1}|; `{variance,jitter}_{mean,max,min}`
with `_persample` (B, S): that reduction over the limbs (the jitter's also over the steps), and without a suffix (B,):
the same reduction over the samples too; jitter_{mean,max,min}_limb (B, S, L) the reduction over the steps alone.
error_limb (B, S, L) the mean over the frames of |target_len - len|, error_persample (B, S) its mean over the limbs,
error_{mean,max,min} (B,) over the samples; the error fields are None without a target."""


def _check_mode(mode, allowed, who):
    if mode not in allowed:  # the reference asserts (body_realism.py:42, :56, :87)
        raise ValueError(f"{who}: mode {mode!r} not supported, expected one of {list(allowed)}")


def _limb_stats(pred, limbseq, target, want):
    """One sd_limb_stats call computing the groups in `want` (a subset of 'limb', 'sample', 'seq', 'steps', 'diff');
    -> dict of the raw output arrays (absent groups None) and the shape."""
    p = _device_tensor(pred, "pred")
    if p.dim() != 5 or p.shape[4] != 3:
        raise ValueError(f"limb statistics: pred (B, S, T, J, 3) expected, got {tuple(p.shape)}")
    B, S, T, J, _ = p.shape
    g = None
    if target is not None:
        g = _device_tensor(target, "target")
        if tuple(g.shape) != (B, T, J, 3):
            raise ValueError(f"limb statistics: target {(B, T, J, 3)} expected for pred {tuple(p.shape)}, got {tuple(g.shape)}")
    limbs, L = _int_table(limbseq, "limbseq")
    dev = p.device
    f32 = dict(device=dev, dtype=torch.float32)
    o = {
        "limb": torch.empty(5, B, S, L, **f32) if "limb" in want else None,
        "sample": torch.empty(7, B, S, **f32) if "sample" in want else None,
        "scratch": torch.empty(7, B, S, device=dev, dtype=torch.float64) if "seq" in want else None,
        "seq": torch.empty(9, B, **f32) if "seq" in want else None,
        "steps": torch.empty(B, S, T - 1, L, **f32) if "steps" in want else None,
        "diff": torch.empty(B, S, T - 1, L, **f32) if "diff" in want else None,
    }
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(_lib.lib().sd_limb_stats(p.data_ptr(), _lib.ptr(g), B, S, T, J, limbs, L, *(_lib.ptr(o[k]) for k in (
        "limb", "sample", "scratch", "seq", "steps", "diff")), stream))
    return o


def limb_stats(pred: torch.Tensor, limbseq, target=None) -> LimbStats:
    """Every limb-length statistic of the validation pass from one launch sequence and one read of pred
    (B, S, T, J, 3); limbseq (L, 2) joint indices (`skeletons.limbseq`); target (B, T, J, 3) or None (then the
    error fields are None).  Float64 inside; the variance over the frames is combined from per-tile sums of
    squares about the tile's mean, never E[x^2] - mean^2.  -> `LimbStats`."""
    o = _limb_stats(pred, limbseq, target, {"limb", "sample", "seq", "steps"})
    lim, sam, seq = o["limb"], o["sample"], o["seq"]
    var = [x for m in range(3) for x in (sam[m], seq[m])]
    jit = [x for m in range(3) for x in (lim[1 + m], sam[3 + m], seq[3 + m])]
    err = [lim[4], sam[6], seq[6], seq[7], seq[8]] if target is not None else [None] * 5
    return LimbStats(lim[0], *var, o["steps"], *jit, *err)


def _limb_mode(pred, limbseq, mode, if_per_sample, row0, who):
    """`mode` over the limbs (and, without if_per_sample, over the samples) of the variance (row0 0) or jitter (row0 3)."""
    _check_mode(mode, _LIMB_MODES, who)
    m = _LIMB_MODES.index(mode)
    if if_per_sample:
        return _limb_stats(pred, limbseq, None, {"sample"})["sample"][row0 + m]
    return _limb_stats(pred, limbseq, None, {"seq"})["seq"][row0 + m]


def limb_length_variance(pred, limbseq, mode="mean", if_per_sample=False, **kwargs):
    """body_realism.py:50-77: the unbiased variance over the frames of every limb's length, pred (B, S, T, J, 3):
    mode 'none' (B, S, L); 'mean' / 'max' / 'min' over the limbs (B, S) with if_per_sample, else over the samples
    too (B,).  The `LLVar` column of the diffusion loop's validation (train_utils.py:108).  T == 1 gives NaN."""
    if mode == "none":
        return _limb_stats(pred, limbseq, None, {"limb"})["limb"][0]
    return _limb_mode(pred, limbseq, mode, if_per_sample, 0, "limb_length_variance")


def limb_length_jitter(pred, limbseq, mode="mean", if_per_sample=False, **kwargs):
    """body_realism.py:79-107: |len_t - len_{t-1}| of every limb: mode 'none' (B, S, T - 1, L); 'mean' / 'max' /
    'min' over the limbs and steps (B, S) with if_per_sample, else over the samples too (B,).  'max' / 'min' of a
    single frame have nothing to reduce (the reference's `max` over an empty axis raises): ValueError."""
    _check_mode(mode, _LIMB_MODES, "limb_length_jitter")
    if mode == "none":
        return _limb_stats(pred, limbseq, None, {"steps"})["steps"]
    if mode in ("max", "min") and pred.shape[2] < 2:
        raise ValueError(f"limb_length_jitter: mode {mode!r} needs at least 2 frames, pred has {pred.shape[2]}")
    return _limb_mode(pred, limbseq, mode, if_per_sample, 3, "limb_length_jitter")


def limb_length_error(target, pred, limbseq, mode="mean", **kwargs):
    """body_realism.py:32-48: the mean over limbs and frames of |target limb length - predicted limb length|,
    then `mode` ('mean' / 'max' / 'min') over the samples -> (B,)."""
    _check_mode(mode, _LIMB_MODES[:3], "limb_length_error")
    return _limb_stats(pred, limbseq, target, {"seq"})["seq"][(6, 7, 8)[_LIMB_MODES.index(mode)]]


def limb_length_variation_difference_wrtGT(target, pred, limbseq, mode="mean", **kwargs):
    """body_realism.py:15-29: limb_length_jitter of the predictions minus that of the ground truth (as one
    sample), both with `mode`, then the reference's own second reduction: over the last axis of the (B,) values,
    i.e. over the batch, and `unsqueeze(0)` -> (1,); mode 'none' -> (B, S, T - 1, L).  `if_per_sample` is
    limb_length_jitter's, as in the reference ((1, B) then).  The two jitters are subtracted in float64."""
    _check_mode(mode, _LIMB_MODES, "limb_length_variation_difference_wrtGT")
    if mode == "none":  # subtracted in float64 inside the kernel, rounded once
        return _limb_stats(pred, limbseq, target, {"diff"})["diff"]
    if mode in ("max", "min") and pred.shape[2] < 2:
        raise ValueError(f"limb_length_variation_difference_wrtGT: mode {mode!r} needs at least 2 frames, pred has "
                         f"{pred.shape[2]}")

    def over_last(v):
        return v.mean(-1) if mode == "mean" else (v.max(-1).values if mode == "max" else v.min(-1).values)

    def jitter64(x):  # the kernel's float64 per-sample values, so the difference below is rounded once
        v = _limb_stats(x, limbseq, None, {"seq"})["scratch"][3 + _LIMB_MODES.index(mode)]  # (B, S)
        return v if kwargs.get("if_per_sample", False) else over_last(v)

    p, g = jitter64(pred), jitter64(target.unsqueeze(1))
    return (over_last(p) - over_last(g)).to(torch.float32).unsqueeze(0)


# ---- streaming per-frame MPJPE and FDE (sd_frame_error_update) ---------------------------------------
def format_metric_time_table(metric: torch.Tensor) -> torch.Tensor:
    """metrics/utils.py:5-10: the rows 0, 30, 60, ... (at most 16) of a profile whose axis 0 is time."""
    steps = [i * 30 for i in range(16) if i * 30 < len(metric)]
    return torch.stack([metric[t] for t in steps], dim=0)


class _FrameErrorAccumulator:
    """State of the sum over the rows of ||pred - target|| per (frame, joint) of a frame window: float64 (nframes,
    joints) and an int64 row count on `device`.  On a ROCm device `update` is one sd_frame_error_update launch
    (after sd_best_sample for `best=True`); on the CPU (a state for `merge` / `all_reduce`, or a host validation)
    the same row-ordered float64 sums are formed with torch ops."""

    _name = "frame error"

    def __init__(self, device=None):
        self.device = torch.device(device or "cpu")
        self.sum = None  # (nframes, J) once the first update gives the shape
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.sum = None
        self.count.zero_()

    def _window(self, frames: int):
        raise NotImplementedError

    def _state(self, nframes: int, joints: int) -> torch.Tensor:
        if self.sum is None:
            self.sum = torch.zeros(nframes, joints, dtype=torch.float64, device=self.device)
        elif tuple(self.sum.shape) != (nframes, joints):
            raise ValueError(f"{self._name}: a batch of {(nframes, joints)} (frames, joints) after batches of "
                             f"{tuple(self.sum.shape)}")
        return self.sum

    def update(self, pred: torch.Tensor, target: torch.Tensor, idx=None, best: bool = False) -> None:
        """pred (rows, frames, joints, 3) or (rows, samples, frames, joints, 3), target (rows, frames, joints, 3).
        With several samples give `idx` (rows,) int64, the sample of every row (`metrics.best_sample`'s idx), or
        `best=True`, which takes the sample closest to the target (sd_best_sample); the chosen future is read
        where it lies.  Nothing is copied to the host."""
        if not torch.is_tensor(pred) or not torch.is_tensor(target):
            raise ValueError(f"{self._name}: pred and target must be tensors")
        if pred.dim() == 4:
            pred = pred.unsqueeze(1)
        if pred.dim() != 5 or pred.shape[4] != 3 or target.dim() != 4 or \
                tuple(target.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
            raise ValueError(f"{self._name}: pred (rows, [samples,] frames, joints, 3) and target (rows, frames, joints, 3) "
                             f"expected, got {tuple(pred.shape)} and {tuple(target.shape)}")
        R, S, T, J, _ = pred.shape
        if idx is not None and best:
            raise ValueError(f"{self._name}: give idx or best=True, not both")
        if idx is None and not best and S != 1:
            raise ValueError(f"{self._name}: pred has {S} samples: give idx (rows,) or best=True")
        frame0, nframes = self._window(T)
        state = self._state(nframes, J)
        if R == 0:
            return
        if self.device.type == "cuda":
            p, g = _device_tensor(pred, "pred"), _device_tensor(target, "target")
            if best:
                idx = _best_sample(p, g, None, False, True, False)[2]
            if idx is not None:
                idx = torch.as_tensor(idx).to(device=p.device, dtype=torch.int64).reshape(-1).contiguous()
                if idx.numel() != R:
                    raise ValueError(f"{self._name}: {idx.numel()} indices for {R} rows")
            stream = torch.cuda.current_stream(p.device).cuda_stream
            check(_lib.lib().sd_frame_error_update(p.data_ptr(), g.data_ptr(), _lib.ptr(idx), R, S, T, J, frame0, nframes,
                                                   state.data_ptr(), self.count.data_ptr(), stream))
            return
        p = pred.detach().to(self.device, torch.float32).to(torch.float64)
        g = target.detach().to(self.device, torch.float32).to(torch.float64)
        if best:
            idx = (p - g.unsqueeze(1)).norm(dim=-1).mean(-1).mean(-1).min(dim=-1).indices
        if idx is None:
            idx = torch.zeros(R, dtype=torch.int64)
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int64).reshape(-1)
        if idx.numel() != R:
            raise ValueError(f"{self._name}: {idx.numel()} indices for {R} rows")
        ok = (idx >= 0) & (idx < S)
        chosen = p[torch.arange(R), idx.clamp(0, S - 1), frame0:frame0 + nframes]
        err = (chosen - g[:, frame0:frame0 + nframes]).norm(dim=-1)
        err[~ok] = float("nan")  # the kernel's rule for an index that is no sample
        for r in range(R):  # the kernel's order: the rows ascending
            state += err[r]
        self.count += R

    def merge(self, other):
        if other.sum is not None:
            self._state(*other.sum.shape).add_(other.sum.to(self.device))
        self.count += other.count.to(self.device)
        return self

    def all_reduce(self, group=None):
        """Sum the states over the ranks; every rank must have seen a batch (the shape is the state's)."""
        import torch.distributed as dist

        if self.sum is None:
            raise SkelDiffError(f"{self._name}: all_reduce before any update on this rank (the state's shape is unknown)")
        dist.all_reduce(self.sum, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.count, op=dist.ReduceOp.SUM, group=group)
        return self

    def _mean(self) -> torch.Tensor:
        """(nframes, joints) float64 on the host: the one copy"""
        if self.sum is None:
            raise SkelDiffError(f"{self._name} must have at least one example before it can be computed.")
        flat = torch.cat([self.sum.reshape(-1), self.count.to(torch.float64)]).cpu()
        return (flat[:-1] / flat[-1]).reshape(self.sum.shape)


class MPJPEAccumulator(_FrameErrorAccumulator):
    """The reference's `MeanPerJointPositionError` (src/metrics/ignite_mpjpe.py) without keeping the split's
    predictions: `compute` is the mean over the rows of the per-joint distance, then over the joints unless
    keep_joint_dim, then the time table (`format_metric_time_table`) with keep_time_dim, else the mean over the
    frames: a float64 host tensor."""

    _name = "MeanPerJointPositionError"

    def __init__(self, keep_time_dim: bool = True, keep_joint_dim: bool = False, device=None):
        super().__init__(device)
        self.keep_time_dim, self.keep_joint_dim = keep_time_dim, keep_joint_dim

    def _window(self, frames: int):
        return 0, frames

    def compute(self) -> torch.Tensor:
        ret = self._mean()
        if not self.keep_joint_dim:
            ret = ret.mean(dim=-1)
        return format_metric_time_table(ret) if self.keep_time_dim else ret.mean(0)


class FDEAccumulator(_FrameErrorAccumulator):
    """The reference's `FinalDisplacementError` (src/metrics/ignite_fde.py): the mean over rows and joints of the
    last frame's per-joint distance, a 0-dim float64 host tensor."""

    _name = "FinalDisplacementError"

    def _window(self, frames: int):
        return frames - 1, 1

    def compute(self) -> torch.Tensor:
        return self._mean().mean()


# ---- FID (sd_fid_features + sd_fid_stats_update) -----------------------------------------
_FID_KEYS = ("recurrent.weight_ih_l0", "recurrent.weight_hh_l0", "recurrent.bias_ih_l0", "recurrent.bias_hh_l0",
             "recurrent.weight_ih_l1", "recurrent.weight_hh_l1", "recurrent.bias_ih_l1", "recurrent.bias_hh_l1",
             "linear1.weight", "linear1.bias")
FID_HIDDEN = 128


class FIDClassifier:
    """The reference's `ClassifierForFID` (src/metrics/fid_classifier.py:5-57) as far as FID uses it:
    `get_fid_features`, i.e. nn.GRU(input_size, 128, 2) over the frames and tanh(linear1(h_last)), as
    one persistent HIP launch per call (sd_fid_features).  Built from the reference's state_dict
    (`recurrent.weight_ih_l0` ... `recurrent.bias_hh_l1`, `linear1.*`; `linear2.*` is accepted and
    unused: FID does not read the class scores)."""

    def __init__(self, state_dict, device):
        self.device = torch.device(device)
        missing = [k for k in _FID_KEYS if k not in state_dict]
        if missing:
            raise KeyError(f"FIDClassifier: state_dict lacks {missing}")
        self._w = {k: state_dict[k].detach().to(self.device, torch.float32).contiguous() for k in _FID_KEYS}
        self.hidden_size = int(self._w["recurrent.weight_hh_l0"].shape[1])
        self.input_size = int(self._w["recurrent.weight_ih_l0"].shape[1])
        self.feat_size = int(self._w["linear1.weight"].shape[0])
        shapes = {"recurrent.weight_ih_l0": (3 * self.hidden_size, self.input_size), "linear1.weight": (self.feat_size, self.hidden_size),
                  "linear1.bias": (self.feat_size,)}
        for k in _FID_KEYS:
            want = shapes.get(k, (3 * self.hidden_size, self.hidden_size) if "weight" in k else (3 * self.hidden_size,))
            if tuple(self._w[k].shape) != want:
                raise ValueError(f"FIDClassifier: {k} has shape {tuple(self._w[k].shape)}, expected {want}")
        self._desc = _lib.SDFidClassifierDesc(self.input_size, self.hidden_size, self.feat_size,
                                              *(self._w[k].data_ptr() for k in _FID_KEYS))
        self._ws = None

    def initHidden(self, num_samples: int) -> torch.Tensor:
        """fid_classifier.py:56-57: a fresh draw from torch's generator of the device per call."""
        return torch.randn(2, num_samples, self.hidden_size, device=self.device)

    def features(self, x: torch.Tensor, hidden_unit=None) -> torch.Tensor:
        """x (..., frames, J, 3) or (rows, frames, input_size), as the pipeline holds it (a contiguous
        float32 tensor is read in place) -> (rows, feat_size) float32.  hidden_unit (2, rows, 128) is
        used as given; None draws `initHidden(rows)`."""
        if self.device.type != "cuda" or not torch.is_tensor(x) or x.device.type != "cuda":
            raise SkelDiffError("FIDClassifier: the classifier runs on the MI355X HIP engine only; build it on, and "
                                "pass, a ROCm device")
        if x.dim() >= 4 and x.shape[-1] * x.shape[-2] == self.input_size:
            rows, frames = _flat(x.shape[:-3]), int(x.shape[-3])
        elif x.dim() == 3 and x.shape[-1] == self.input_size:
            rows, frames = int(x.shape[0]), int(x.shape[1])
        else:
            raise ValueError(f"FIDClassifier: (..., frames, J, 3) with 3 J = {self.input_size} or (rows, frames, "
                             f"{self.input_size}) expected, got {tuple(x.shape)}")
        x = _device_tensor(x, "motion")
        if hidden_unit is None:
            hidden_unit = self.initHidden(rows)
        h0 = _device_tensor(hidden_unit, "hidden_unit")
        if tuple(h0.shape) != (2, rows, self.hidden_size):
            raise ValueError(f"FIDClassifier: hidden_unit {tuple(h0.shape)}, expected {(2, rows, self.hidden_size)}")
        L = _lib.lib()
        if self._ws is None:
            self._ws = torch.empty(max(int(L.sd_fid_workspace_bytes(ctypes.byref(self._desc), rows)), 1), device=self.device,
                                   dtype=torch.uint8)
        feats = torch.empty(rows, self.feat_size, device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(L.sd_fid_features(ctypes.byref(self._desc), x.data_ptr(), rows, frames, h0.data_ptr(), feats.data_ptr(),
                                self._ws.data_ptr(), self._ws.numel(), stream))
        return feats

    def get_fid_features(self, motion_sequence: torch.Tensor, hidden_unit=None) -> torch.Tensor:
        """fid_classifier.py:38-53 with its argument layout: motion_sequence (b, input_size, frames).
        The permuted view the reference's storer passes (fid.py:113, :117) is read where it lies."""
        return self.features(motion_sequence.permute(0, 2, 1), hidden_unit)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """fid.py:17-68 `_calculate_frechet_distance` on the host in float64, without scipy:
    |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), the last trace as the sum of the square roots of
    the eigenvalues of S1 S2 (real parts, clamped at 0: the product of two PSD matrices has real
    non-negative eigenvalues up to rounding)."""
    mu1, mu2 = (torch.atleast_1d(torch.as_tensor(m)).cpu() for m in (mu1, mu2))  # float32 means subtract in float32
    s1, s2 = (torch.atleast_2d(torch.as_tensor(s, dtype=torch.float64)).cpu() for s in (sigma1, sigma2))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert s1.shape == s2.shape, "Training and test covariances have different dimensions"
    diff = (mu1 - mu2).to(torch.float64)
    ev = torch.linalg.eigvals(s1 @ s2).real.clamp_min(0.0)
    return float(diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2.0 * ev.sqrt().sum())


class FIDAccumulator:
    """The reference's `MetricStorerFID` (fid.py:91-129) without the host: `update` queues the two
    feature passes and folds their activations into two float64 states (count, sum x, sum x x^T) on
    the device; `compute` copies the 2 x (1 + feat + feat^2) doubles once.  `classifier` None (with
    `feat_size`, `device`) gives a statistics-only accumulator for `merge` / `all_reduce`."""

    def __init__(self, classifier=None, feat_size=None, device=None):
        self.classifier = classifier
        self.feat_size = int(classifier.feat_size if classifier is not None else feat_size)
        self.device = torch.device(classifier.device if classifier is not None else (device or "cpu"))
        n = 1 + self.feat_size + self.feat_size ** 2
        self.state_pred = torch.zeros(n, dtype=torch.float64, device=self.device)
        self.state_gt = torch.zeros(n, dtype=torch.float64, device=self.device)

    def reset(self) -> None:
        self.state_pred.zero_()
        self.state_gt.zero_()

    def _fold(self, feats: torch.Tensor, state: torch.Tensor) -> None:
        L = _lib.lib()
        rows = feats.shape[0]
        ws = torch.empty(max(int(L.sd_fid_stats_workspace_bytes(rows, self.feat_size)), 1), device=feats.device,
                         dtype=torch.uint8)
        stream = torch.cuda.current_stream(feats.device).cuda_stream
        check(L.sd_fid_stats_update(feats.data_ptr(), rows, self.feat_size, state.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream))

    def update_features(self, pred_feats=None, gt_feats=None) -> None:
        """Fold (rows, feat_size) float32 device activations into the states."""
        for f, st in ((pred_feats, self.state_pred), (gt_feats, self.state_gt)):
            if f is not None:
                f = _device_tensor(f, "features")
                if f.dim() != 2 or f.shape[1] != self.feat_size:
                    raise ValueError(f"FIDAccumulator: features (rows, {self.feat_size}) expected, got {tuple(f.shape)}")
                self._fold(f, st)

    def update(self, pred, target, hidden_unit_pred=None, hidden_unit_gt=None) -> None:
        """fid.py:106-123: pred (B, S, T, J, 3), target (B, T, J, 3).  The predictions' features come
        first, then the ground truth's (the reference's call order, so its randn order).  Everything
        is queued on the current stream; nothing is copied to the host."""
        if self.classifier is None:
            raise SkelDiffError("FIDAccumulator: built without a classifier (statistics only)")
        fp = self.classifier.features(pred, hidden_unit_pred)
        fg = self.classifier.features(target, hidden_unit_gt)
        self._fold(fp, self.state_pred)
        self._fold(fg, self.state_gt)

    def merge(self, other: "FIDAccumulator") -> "FIDAccumulator":
        self.state_pred += other.state_pred.to(self.device)
        self.state_gt += other.state_gt.to(self.device)
        return self

    def all_reduce(self, group=None) -> "FIDAccumulator":
        """Sum the states over the ranks (RCCL for device states, gloo for host ones)."""
        import torch.distributed as dist

        both = torch.stack([self.state_pred, self.state_gt])
        dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
        self.state_pred.copy_(both[0])
        self.state_gt.copy_(both[1])
        return self

    @staticmethod
    def statistics(state):
        """(mu float32, sigma float64) of one state: `np.mean` of float32 activations
        (a float32 result) and `np.cov(rowvar=False)` (float64, unbiased), fid.py:7-11."""
        st = torch.as_tensor(state).detach().to("cpu", torch.float64)
        F = int(round((-1 + (1 + 4 * (st.numel() - 1)) ** 0.5) / 2))
        n = float(st[0])
        if n < 2:
            raise ValueError(f"FID needs at least 2 rows per side for a covariance, got {int(n)}")
        sx, sxx = st[1:1 + F], st[1 + F:].reshape(F, F)
        mean = sx / n
        sigma = (sxx - torch.outer(sx, sx) / n) / (n - 1.0)
        return mean.to(torch.float32), sigma

    def compute(self) -> float:
        """fid.py:125-129: `fid(gt activations, pred activations)` as a Python float."""
        both = torch.stack([self.state_gt, self.state_pred]).cpu()  # the one device-to-host copy
        mu_g, sg_g = self.statistics(both[0])
        mu_p, sg_p = self.statistics(both[1])
        return frechet_distance(mu_g, sg_g, mu_p, sg_p)


# ---- APDE (the table: multimodal_gt.MultimodalGT.gt_apd) -----------------------------------------
class APDEAccumulator:
    """The reference's `MetricStorerAPDE` (src/metrics/apde.py:9-48) on the device: the mean over the test
    segments of |APD(pred) - APD(multimodal ground truth)|, skipping segments whose ground-truth APD is 0
    (they become NaN, apde.py:18) or NaN.  `gt_apd` is the per-segment table (`MultimodalGT.gt_apd`, or
    `from_csv` for the reference's mmapd_GT.csv) in the order the evaluation visits the segments; `ids`
    (optional) the segment number of every entry, for updates by index when that order is not 0, 1, 2, ...
    State: a float64 sum and an int64 count on `device`; torch ops only (not a hot path)."""

    def __init__(self, gt_apd, device=None, ids=None):
        g = torch.as_tensor(gt_apd)
        self.device = torch.device(device) if device is not None else g.device
        g = g.detach().to(self.device, torch.float64).reshape(-1)
        self.gt_apd = torch.where(g == 0, torch.full_like(g, float("nan")), g)
        self._pos = None
        if ids is not None:
            ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
            if ids.numel() != g.numel():
                raise ValueError(f"APDEAccumulator: {ids.numel()} ids for {g.numel()} values")
            if not torch.equal(ids.cpu(), torch.arange(g.numel())):
                self._pos = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int64)
                self._pos[ids.cpu()] = torch.arange(g.numel())
                self._pos = self._pos.to(self.device)
        self.sum = torch.zeros((), dtype=torch.float64, device=self.device)
        self.count = torch.zeros((), dtype=torch.int64, device=self.device)
        self.index = 0

    @classmethod
    def from_csv(cls, path, device="cpu") -> "APDEAccumulator":
        """apde.py:17: the `gt_APD` column of an `id,gt_APD` file (the first column is the index), rows in file order."""
        import csv

        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        head = rows[0]
        if "gt_APD" not in head:
            raise ValueError(f"{path}: no gt_APD column in {head}")
        c = head.index("gt_APD")
        body = [r for r in rows[1:] if r]
        values = [float(r[c]) if r[c] != "" else float("nan") for r in body]
        return cls(torch.tensor(values, dtype=torch.float64), device, ids=[int(r[0]) for r in body])

    def reset(self) -> None:
        self.sum.zero_()
        self.count.zero_()
        self.index = 0

    def update(self, apd_pred: torch.Tensor, segment_idx=None) -> None:
        """apde.py:29-41: apd_pred (B,) the batch's `metrics.apd(pred)`.  Without segment_idx the next B table
        entries are consumed, as the reference; with it (segment numbers; a list or a tensor) entry by index,
        for a sharded evaluation.  Nothing is copied to the host."""
        a = torch.as_tensor(apd_pred).detach().to(self.device, torch.float64).reshape(-1)
        B = a.numel()
        if segment_idx is None:
            if self.index + B > self.gt_apd.numel():
                raise ValueError(f"APDEAccumulator: {self.index + B} predictions for a table of {self.gt_apd.numel()}")
            g = self.gt_apd[self.index:self.index + B]
            self.index += B
        else:
            idx = torch.as_tensor(segment_idx, dtype=torch.int64).to(self.device).reshape(-1)
            if idx.numel() != B:
                raise ValueError(f"APDEAccumulator: {idx.numel()} indices for {B} predictions")
            g = self.gt_apd[idx if self._pos is None else self._pos[idx]]
        err = (a - g).abs()
        ok = ~torch.isnan(err)
        self.sum += torch.where(ok, err, torch.zeros_like(err)).sum()
        self.count += ok.sum()

    def merge(self, other: "APDEAccumulator") -> "APDEAccumulator":
        self.sum += other.sum.to(self.device)
        self.count += other.count.to(self.device)
        return self

    def all_reduce(self, group=None) -> "APDEAccumulator":
        """Sum the states over the ranks (RCCL for device states, gloo for host ones); a count is exact in float64."""
        import torch.distributed as dist

        both = torch.stack([self.sum, self.count.to(torch.float64)])
        dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
        self.sum.copy_(both[0])
        self.count.copy_(both[1].to(torch.int64))
        return self

    def compute(self) -> float:
        """apde.py:43-48: sum / count as a Python float (NaN before any counted segment): the one copy to the host."""
        s, c = torch.stack([self.sum, self.count.to(torch.float64)]).cpu().tolist()
        return s / c if c else float("nan")


# ---- diversity ranking (sd_diverse_rank) -----------------------------------------------------------
MAX_RANK_SAMPLES = 255  # sd::rank::kMaxPoints - 1
DiverseRank = collections.namedtuple("DiverseRank", ["idx", "score", "closest"])
DiverseRank.__doc__ = """What `diverse_rank` returns: idx (B, n) int64 the picked samples in pick order, score (B, n)
float32 each pick's distance to the set chosen before it, closest (B,) int64 the sample nearest the target
(None without from_closest).  Device tensors."""


def _rank(pred, target, n, from_closest, want_dist=False):
    if not torch.is_tensor(pred) or not torch.is_tensor(target) or pred.dim() < 3 or target.dim() != pred.dim() - 1 \
            or target.shape[0] != pred.shape[0] or tuple(target.shape[1:]) != tuple(pred.shape[2:]):
        raise ValueError(f"diverse_rank: pred (B, S, ...) and target (B, ...) expected, got "
                         f"{tuple(getattr(pred, 'shape', ()))} and {tuple(getattr(target, 'shape', ()))}")
    B, S = int(pred.shape[0]), int(pred.shape[1])
    p = _device_tensor(pred.reshape(B, S, _flat(pred.shape[2:])), "pred")
    g = _device_tensor(target.reshape(B, _flat(target.shape[1:])), "target")
    n = int(n)
    dev, L = p.device, _lib.lib()
    idx = torch.empty(B, max(n, 0), device=dev, dtype=torch.int64)
    score = torch.empty(B, max(n, 0), device=dev, dtype=torch.float32)
    closest = torch.empty(B, device=dev, dtype=torch.int64) if from_closest else None
    dist = torch.empty(B, S + 1, S + 1, device=dev, dtype=torch.float32) if want_dist else None
    ws = torch.empty(max(int(L.sd_diverse_rank_workspace_bytes(B, S)), 1), device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(L.sd_diverse_rank(p.data_ptr(), g.data_ptr(), B, S, p.shape[2], n, int(bool(from_closest)), idx.data_ptr(),
                            score.data_ptr(), _lib.ptr(closest), _lib.ptr(dist), ws.data_ptr(), ws.numel(), stream))
    return DiverseRank(idx, score, closest), dist


def diverse_rank(pred: torch.Tensor, target: torch.Tensor, n: int, from_closest: bool = False) -> DiverseRank:
    """Farthest-point greedy over each sequence's samples (ranking.py:3-40): pred (B, S, ...), target (B, ...)
    -> DiverseRank.  Starting from the target (or, with from_closest, from the sample nearest to it,
    ranking.py:42-63), each pick is the sample farthest from everything chosen so far, the lowest index on
    a tie; a NaN sample is picked last (the reference raises).  Two launches on the current stream,
    nothing is copied to the host.  S <= 255, 1 <= n <= S."""
    return _rank(pred, target, n, from_closest)[0]


def find_samples_maxapd_wrtGT(pred: torch.Tensor, target: torch.Tensor, num_chosen_samples: int = 5):
    """ranking.py:30-40: (None, idx (B, num_chosen_samples) int64 on the device); `idx.tolist()` is the
    reference's list of lists."""
    return None, _rank(pred, target, num_chosen_samples, False)[0].idx


def get_closest_and_nfurthest_maxapd(y_pred: torch.Tensor, y_gt: torch.Tensor, nsamples: int):
    """ranking.py:42-63: y_pred (S, T, J, 3), y_gt (T, J, 3) -> (pred_closest (T, J, 3), sorted_preds
    (nsamples, T, J, 3), idx (nsamples,) int64): the sample closest to the ground truth, then the nsamples
    most mutually distant ones starting from it.  With a leading batch axis on both, every result has it
    too.  The gathers are device ops; nothing is copied to the host."""
    batched = y_pred.dim() == 5
    assert y_pred.dim() in (4, 5) and y_pred.shape[-1] == 3, f"Expected SxTxJx3 tensors, got {y_pred.dim()}"
    assert y_gt.dim() == y_pred.dim() - 1 and y_gt.shape[-2:] == y_pred.shape[-2:], f"Expected TxJx3 tensors, got {y_gt.dim()}"
    p, g = (y_pred, y_gt) if batched else (y_pred.unsqueeze(0), y_gt.unsqueeze(0))
    r = _rank(p, g, nsamples, True)[0]
    rows = torch.arange(p.shape[0], device=r.idx.device)
    pred_closest, sorted_preds = p[rows, r.closest], p[rows.unsqueeze(1), r.idx]
    if batched:
        return pred_closest, sorted_preds, r.idx
    return pred_closest[0], sorted_preds[0], r.idx[0]


# ---- class-wise CMD (sd_class_sum) and the metric storers ---------------------------------------
class CMDAccumulator:
    """The reference's `CMDMetricStorer` + `resolve_cmd` (src/metrics/cmd.py:15-57) without the per-batch
    host copies: float64 sums (C, W) of the motion profiles per class, int64 counts (C) and an int64 total
    on `device`.  `mean_motion_per_class` holds the dataset's mean motion per class, in class-index order.
    On a ROCm device `update` is one sd_class_sum launch; on the CPU (a state for `merge` / `all_reduce`,
    or a host evaluation) the same row-ordered float64 sums are formed with torch ops."""

    def __init__(self, mean_motion_per_class, device=None):
        self.ref = [float(v) for v in mean_motion_per_class]
        self.classes = len(self.ref)
        if self.classes < 1:
            raise ValueError("CMDAccumulator: mean_motion_per_class is empty")
        self.device = torch.device(device or "cpu")
        self.sum = None  # (C, W) once the first update gives W
        self.count = torch.zeros(self.classes, dtype=torch.int64, device=self.device)
        self.total = torch.zeros(1, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.sum = None
        self.count.zero_()
        self.total.zero_()

    def _state(self, width: int) -> torch.Tensor:
        if self.sum is None:
            self.sum = torch.zeros(self.classes, width, dtype=torch.float64, device=self.device)
        elif self.sum.shape[1] != width:
            raise ValueError(f"CMDAccumulator: profiles of {width} steps after profiles of {self.sum.shape[1]}")
        return self.sum

    def update(self, motion: torch.Tensor, class_idx) -> None:
        """motion (B, W) the batch's `motion_for_cmd(pred)`, class_idx (B,) class indices (tensor, array or
        list).  Nothing is copied to the host."""
        m = torch.as_tensor(motion).detach()
        if m.dim() != 2:
            raise ValueError(f"CMDAccumulator: motion (B, W) expected, got {tuple(m.shape)}")
        c = torch.as_tensor(class_idx).to(dtype=torch.int64).reshape(-1)
        if c.numel() != m.shape[0]:
            raise ValueError(f"CMDAccumulator: {c.numel()} class indices for {m.shape[0]} rows")
        m = m.to(self.device, torch.float32).contiguous()
        c = c.to(self.device).contiguous()
        s = self._state(int(m.shape[1]))
        if m.shape[0] == 0:
            return
        if self.device.type == "cuda":
            stream = torch.cuda.current_stream(self.device).cuda_stream
            check(_lib.lib().sd_class_sum(m.data_ptr(), c.data_ptr(), m.shape[0], m.shape[1], self.classes, s.data_ptr(),
                                          self.count.data_ptr(), self.total.data_ptr(), stream))
            return
        md = m.to(torch.float64)
        for r in range(m.shape[0]):  # the kernel's order: per class the rows ascending
            k = int(c[r])
            if 0 <= k < self.classes:
                s[k] += md[r]
                self.count[k] += 1
        self.total += m.shape[0]

    def merge(self, other: "CMDAccumulator") -> "CMDAccumulator":
        if other.sum is not None:
            self._state(int(other.sum.shape[1])).add_(other.sum.to(self.device))
        self.count += other.count.to(self.device)
        self.total += other.total.to(self.device)
        return self

    def all_reduce(self, group=None) -> "CMDAccumulator":
        """Sum the states over the ranks; every rank must have seen a batch (the width is the state's)."""
        import torch.distributed as dist

        if self.sum is None:
            raise SkelDiffError("CMDAccumulator.all_reduce: no update yet on this rank (the profile width is unknown)")
        dist.all_reduce(self.sum, op=dist.ReduceOp.SUM, group=group)
        ints = torch.cat([self.count, self.total])
        dist.all_reduce(ints, op=dist.ReduceOp.SUM, group=group)
        self.count.copy_(ints[:-1])
        self.total.copy_(ints[-1:])
        return self

    def _host(self):
        """(sums (C, W) f64, counts (C) f64, total) on the host: the one copy"""
        if self.sum is None:
            raise SkelDiffError("CMDAccumulator: needs at least one update before it can be computed")
        flat = torch.cat([self.sum.reshape(-1), self.count.to(torch.float64), self.total.to(torch.float64)]).cpu()
        C, W = self.sum.shape
        return flat[:C * W].reshape(C, W), flat[C * W:C * W + C], float(flat[-1])

    def motion_per_class(self) -> torch.Tensor:
        """cmd.py:22-29: (C, W) float64 on the host, the mean profile per class, zeros for an empty class."""
        s, n, _ = self._host()
        return torch.where(n.unsqueeze(1) > 0, s / n.clamp_min(1.0).unsqueeze(1), torch.zeros_like(s))

    def compute(self) -> float:
        """cmd.py:24-31: sum over the non-empty classes of cmd(mean profile, class mean motion) * count /
        total, in float64, as a Python float."""
        s, n, total = self._host()
        out = 0.0
        for k in range(self.classes):
            if n[k] > 0:
                out += cmd(s[k] / n[k], self.ref[k]) * (float(n[k]) / total)
        return out


class MetricAccumulator:
    """The reference's `MetricStorer` (src/metrics/metric_storer.py) with a float64 state on the device
    of the values it is fed: return_op 'mean' / 'avg' (sum over the rows / number of rows), 'max', 'min'.
    As the reference's (metric_storer.py:16), 'max' starts at 0 and 'min' at 1000000.  Torch ops only (not
    a hot path); nothing is copied to the host before `compute`."""

    def __init__(self, return_op="mean", device=None):
        assert return_op in ["mean", "avg", "max", "min"]
        self.return_op = return_op
        self.device = torch.device(device) if device is not None else None
        self.reset()

    def _start(self) -> float:
        return 1000000.0 if self.return_op == "min" else 0.0

    def reset(self) -> None:
        self.cumulator = None  # float64 () or (k,), on the first update's device
        self.count = 0         # rows fed (host: shapes are known without a copy)

    def _fold(self, v: torch.Tensor) -> None:
        if self.cumulator is None:
            self.cumulator = torch.full(v.shape, self._start(), dtype=torch.float64, device=v.device)
        if self.return_op in ("mean", "avg"):
            self.cumulator = self.cumulator + v
        elif self.return_op == "max":
            self.cumulator = torch.maximum(self.cumulator, v)
        else:
            self.cumulator = torch.minimum(self.cumulator, v)

    def update(self, values: torch.Tensor) -> None:
        """values (B,) or (B, k): one row per sequence."""
        v = torch.as_tensor(values).detach()
        if v.dim() not in (1, 2):
            raise ValueError(f"MetricAccumulator: values (B,) or (B, k) expected, got {tuple(v.shape)}")
        v = v.to(self.device if self.device is not None else v.device, torch.float64)
        if self.device is None:
            self.device = v.device
        if v.shape[0] == 0:
            return
        if self.return_op in ("mean", "avg"):
            self._fold(v.sum(0))
            self.count += int(v.shape[0])
        else:
            self._fold(v.max(0).values if self.return_op == "max" else v.min(0).values)

    def merge(self, other: "MetricAccumulator") -> "MetricAccumulator":
        assert other.return_op == self.return_op
        if other.cumulator is not None:
            if self.device is None:
                self.device = other.cumulator.device
            self._fold(other.cumulator.to(self.device))
        self.count += other.count
        return self

    def all_reduce(self, group=None) -> "MetricAccumulator":
        """SUM (and the row count), MAX or MIN over the ranks."""
        import torch.distributed as dist

        if self.cumulator is None:
            raise SkelDiffError("MetricAccumulator.all_reduce: no update yet on this rank (the value shape is unknown)")
        if self.return_op in ("mean", "avg"):
            both = torch.cat([self.cumulator.reshape(-1), torch.tensor([float(self.count)], dtype=torch.float64,
                                                                       device=self.cumulator.device)])
            dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
            self.cumulator = both[:-1].reshape(self.cumulator.shape)
            self.count = int(both[-1])
        else:
            dist.all_reduce(self.cumulator, op=dist.ReduceOp.MAX if self.return_op == "max" else dist.ReduceOp.MIN,
                            group=group)
        return self

    def compute(self):
        """metric_storer.py:38-43: a Python float for (B,) values, a float64 host tensor (k,) for (B, k):
        the one copy to the host."""
        if self.cumulator is None:
            raise SkelDiffError("MetricAccumulator must have at least one example before it can be computed.")
        tot = self.cumulator.cpu()
        if self.return_op in ("mean", "avg"):
            tot = tot / self.count
        return float(tot) if tot.dim() == 0 else tot


__all__ = ["lat_apd", "apd", "ade", "fde", "mmade", "mmfde", "cmd", "mpjpe", "best_sample", "get_best_sample_idx",
           "choose_best_sample", "limb_stretching_normed_rmse", "limb_stretching_normed_mean", "limb_jitter_normed_rmse",
           "limb_jitter_normed_mean", "mae", "motion_for_cmd", "realism", "Realism", "FIDClassifier", "FIDAccumulator",
           "frechet_distance", "APDEAccumulator", "diverse_rank", "DiverseRank", "find_samples_maxapd_wrtGT",
           "get_closest_and_nfurthest_maxapd", "CMDAccumulator", "MetricAccumulator", "limb_length_variance",
           "limb_length_jitter", "limb_length_error", "limb_length_variation_difference_wrtGT", "limb_stats", "LimbStats",
           "format_metric_time_table", "MPJPEAccumulator", "FDEAccumulator"]
