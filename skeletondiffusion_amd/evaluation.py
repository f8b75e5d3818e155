"""The reference's evaluation chain on the HIP engine: `get_prediction` (src/eval_prepare_model.py:89-121)
and the long-term rollouts (src/eval_utils.py:44-99), with the reference's signatures and return values.

    get_diffusion_latent_codes(obs, model, num_samples, ...)   past embedding -> sample()
    decode_latent_pred(obs, latent_pred, z_past, model, ...)   latents -> (B, S, pred_length, J, 3)
    get_prediction(obs, model, num_samples, pred_length, ...)  the two in a row
    long_term_prediction_best_every50(...)   draw S futures, keep the one closest to the ground truth,
                                             feed its last observed-length frames back, repeat
    long_term_prediction_best_first50(...)   draw S futures once, then continue each of them
    get_stats_funcs(stats_mode, skeleton_key)   the metric dict of an evaluation loop (src/config_metrics.py:18-53)
    get_fid_storer / get_apde_storer / get_cmd_storer   the dataset-level storers (config_metrics.py:55-69)
    metric_set(stats_mode, skeleton_key, ...)   all of them behind update / all_reduce / compute, the result table
                                             of an evaluation (config_metrics.py:71-96)
    validation_set(kind, skeleton_key, loss_fn)   the validation table of the two training loops behind the same
                                             three calls (src/train_utils.py:56-135 setup_validation_*)

`model` is the (autoencoder, diffusion) pair of `prepare_model`.  Every stage is a HIP kernel sequence
(sd_gru_encode, sd_sample_loop, sd_gru_decode, sd_best_sample); nothing here copies to the host or
synchronises, so the segments of a rollout queue back to back on the stream.
"""
from __future__ import annotations

import math
from functools import partial

import torch

from . import metrics, skeletons


def get_diffusion_latent_codes(obs, model, num_samples=50, diffusion_conditioning=True, sampler_kwargs=None, **kwargs):
    """eval_prepare_model.py:89-104: (latent_pred (bs * num_samples, J, latent), z_past (bs, J, latent)).
    The conditioning goes to sample() once per sequence: the engine repeats `x_cond` rows that divide
    the batch (`cond_repeat`), so `repeat_interleave(num_samples, 0)` is never materialised.
    `sampler_kwargs` may carry the engine's `seed`."""
    autoencoder, diffusion = model
    bs = obs.shape[0]
    sampler_kwargs = sampler_kwargs or {}
    z_past = autoencoder.get_past_embedding(obs)  # z_activation applied
    if diffusion_conditioning:
        latent_pred, _ = diffusion.sample(batch_size=bs * num_samples, x_cond=z_past, **sampler_kwargs)
    else:  # (the reference reads z_past before assigning it on this branch, :102)
        latent_pred, _ = diffusion.sample(batch_size=bs * num_samples, **sampler_kwargs)
    return latent_pred, z_past


def decode_latent_pred(obs, latent_pred, z_past, model, num_samples=50, pred_length=100, **kwargs):
    """eval_prepare_model.py:106-116: (bs, num_samples, pred_length, J, 3).  The decoder reads the last
    two observed frames only, so only those are repeated per sample; it does not read z_past
    (decoder.py:85-104)."""
    autoencoder, _ = model
    bs, _, j, f = obs.shape
    pred = autoencoder.decode(obs[:, -2:].repeat_interleave(num_samples, 0), latent_pred, None, ph=pred_length)
    return pred.view(bs, num_samples, pred_length, j, f)


def get_prediction(obs, model, num_samples=50, pred_length=100, diffusion_conditioning=True, sampler_kwargs=None,
                   **kwargs):
    """eval_prepare_model.py:118-121: obs (bs, obs_length, J, 3) -> (bs, num_samples, pred_length, J, 3)."""
    lat_pred, z_past = get_diffusion_latent_codes(obs, model, num_samples=num_samples,
                                                  diffusion_conditioning=diffusion_conditioning,
                                                  sampler_kwargs=sampler_kwargs, **kwargs)
    return decode_latent_pred(obs, lat_pred, z_past, model, num_samples=num_samples, pred_length=pred_length, **kwargs)


def process_evaluation_pair(target, pred_dict):
    """eval_prepare_model.py:124-134 without the skeleton: the shape assertion, and the inputs back.
    `transform_to_metric_space` stays with the caller (pass a function of your own to the rollouts)."""
    pred, mm_gt, obs = pred_dict["pred"], pred_dict.get("mm_gt"), pred_dict["obs"]
    batch_size, n_samples, seq_length, num_joints, features = pred.shape
    assert features == 3 and list(target.shape) == [batch_size, seq_length, num_joints, features]
    return target, pred, mm_gt, obs


def _segments(config):
    """(number of segments, frames kept of the last one or None): ceil(factor) segments, the last cut
    to int(factor * pred_length) % pred_length frames for a fractional factor (eval_utils.py:51-54)."""
    factor, pred_length = config["long_term_factor"], config["pred_length"]
    n = math.ceil(factor)
    return n, (int(factor * pred_length) % pred_length if int(factor) != factor else None)


def long_term_prediction_best_every50(data, target, extra, get_prediction, process_evaluation_pair=process_evaluation_pair,
                                      num_samples=50, config=None):
    """eval_utils.py:44-67: per segment draw the futures, keep the one closest to the ground truth and
    take its last observed-length frames as the next past.  Selection, best trajectory and next past
    come from one `metrics.best_sample` call; nothing between two segments leaves the device.
    Returns (target, pred, mm_gt, data); pred (B, num_samples, T_total, J, 3) is the best trajectory
    expanded over the sample axis (a view: the reference's `repeat` of identical rows)."""
    new_data = data
    final_pred_data, final_target_data = [], []
    n_past_frames = data.shape[-3]
    n_seg, last_frames = _segments(config)
    pl = config["pred_length"]
    for idx in range(n_seg):
        pred = get_prediction(new_data, extra=extra)  # (batch_size, n_samples, seq_length, num_joints, features)
        if idx == n_seg - 1 and last_frames is not None:
            pred = pred[..., :last_frames, :, :]
        target_m, pred, mm_gt, data_metric_space = process_evaluation_pair(
            target=target[..., idx * pl:(idx + 1) * pl, :, :], pred_dict={"pred": pred, "obs": new_data})
        if idx == 0:
            data = data_metric_space
        # pred[indeces_bool][..., -n_past_frames:, :, :] keeps the whole segment when it is shorter
        _, _, best_pred, tail = metrics.best_sample(pred, target_m, tail=min(n_past_frames, pred.shape[2]))
        final_pred_data.append(best_pred)
        final_target_data.append(target_m)
        new_data = tail
    final_pred_data = torch.cat(final_pred_data, dim=-3)
    pred = final_pred_data.unsqueeze(1).expand(-1, num_samples, -1, -1, -1)
    return torch.cat(final_target_data, dim=-3), pred, mm_gt, data


def long_term_prediction_best_first50(data, target, extra, get_prediction, process_evaluation_pair=process_evaluation_pair,
                                      num_samples=50, config=None):
    """eval_utils.py:69-99: draw num_samples futures once, then continue every one of them with one
    sample each (`get_prediction(..., num_samples=1)` on B * S rows).  Returns (target, pred, mm_gt, data)."""
    new_data = data
    final_pred_data, final_target_data = [], []
    n_seg, last_frames = _segments(config)
    pl = config["pred_length"]
    for idx in range(n_seg):
        if idx == 0:
            pred = get_prediction(new_data, num_samples=num_samples, extra=extra)
        else:
            batch_size, num_samples, seq_length, num_joints, features = new_data.shape
            pred = get_prediction(new_data.reshape(batch_size * num_samples, seq_length, num_joints, features),
                                  num_samples=1, extra=extra)
            pred = pred.reshape(batch_size, num_samples, pl, num_joints, features)
        if idx == n_seg - 1 and last_frames is not None:
            pred = pred[..., :last_frames, :, :]
        target_m, pred, mm_gt, data_metric_space = process_evaluation_pair(
            target=target[..., idx * pl:(idx + 1) * pl, :, :], pred_dict={"pred": pred, "obs": new_data})
        if idx == 0:
            data = data_metric_space
        final_pred_data.append(pred)
        final_target_data.append(target_m)
        new_data = pred[..., -data.shape[-3]:, :, :]  # cut off the first frames
    return torch.cat(final_target_data, dim=-3), torch.cat(final_pred_data, dim=-3), mm_gt, data


def _times_100(fn):
    """config_metrics.py:23-27: the body-realism values are reported in per cent of the limb length."""
    def scaled(*args, **kwargs):
        return fn(*args, **kwargs) * 100
    return scaled


def get_stats_funcs(stats_mode, skeleton_key, **kwargs):
    """config_metrics.py:18-53: name -> metric function of an evaluation loop, every one on the device
    (`skeletondiffusion_amd.metrics`), for stats_mode 'deterministic', 'probabilistic_orig' or
    'probabilistic' (the release setting).  `skeleton_key` names the limb tables
    (`skeletons.limbseq / limb_angles_idx`: 'h36m16', 'amass21', 'freeman17', 'mano51'); the hip is not a
    node (the reference asserts `not if_consider_hip`).  Each function is called as the reference's:
    `fn(pred=..., target=..., mm_gt=..., ...)`."""
    assert not kwargs.get("if_consider_hip", False)
    limbseq, limb_angles_idx = skeletons.limbseq(skeleton_key), skeletons.limb_angles_idx(skeleton_key)
    realism = {
        "StretchMean": partial(_times_100(metrics.limb_stretching_normed_mean), limbseq=limbseq),
        "JitterMean": partial(_times_100(metrics.limb_jitter_normed_mean), limbseq=limbseq),
        "StretchRMSE": partial(_times_100(metrics.limb_stretching_normed_rmse), limbseq=limbseq),
        "JitterRMSE": partial(_times_100(metrics.limb_jitter_normed_rmse), limbseq=limbseq),
    }
    mae = partial(metrics.mae, limbseq=limbseq, limb_angles_idx=limb_angles_idx)
    mode = stats_mode.lower()
    if "deterministic" in mode:
        return {"ADE": metrics.ade, "FDE": metrics.fde, "MAE": mae, "APD": metrics.apd, **realism}
    if mode == "probabilistic_orig":
        return {"APD": metrics.apd, "ADE": metrics.ade, "FDE": metrics.fde, "MMADE": metrics.mmade, "MMFDE": metrics.mmfde}
    if mode == "probabilistic":
        return {"ADE": metrics.ade, "FDE": metrics.fde, "MAE": mae, "MMADE": metrics.mmade, "MMFDE": metrics.mmfde,
                "APD": metrics.apd, **realism}
    raise NotImplementedError(f"stats_mode not implemented: {stats_mode}")


def get_fid_storer(classifier_path=None, if_consider_hip=False, device="cuda", **kwargs):
    """config_metrics.py:58-60 `get_fid_storer` with fid.py:80-89 `get_classifier`, without ignite:
    (a `metrics.FIDAccumulator` over `<classifier_path>/h36m_classifier.pth`, the `(pred, target)`
    selector of the evaluation dict).  `classifier_path` defaults to the reference's
    `precomputed_folder` entry of the config.  Per batch: `acc.update(*select(**out))`; at the end
    `acc.compute()`."""
    from . import checkpoint

    assert not if_consider_hip, "The skeleton should not consider hip to use the classifier."
    path = classifier_path if classifier_path is not None else kwargs["precomputed_folder"]
    acc = metrics.FIDAccumulator(checkpoint.load_fid_classifier(path, device))
    return acc, lambda pred, target, **kwgs: (pred, target)


def get_apde_storer(annotations_folder=None, gt_apd=None, device="cuda", **kwargs):
    """config_metrics.py:55-56 `get_apde_storer` without ignite: (a factory of `metrics.APDEAccumulator`, the
    `pred -> apd(pred)` transform of the evaluation dict).  The table is `gt_apd` (a tensor, e.g.
    `MultimodalGT.gt_apd(futures)`) or `<annotations_folder>/mmapd_GT.csv`, the reference's file.  Per batch:
    `acc.update(transform(**out))`; at the end `acc.compute()`.  The factory takes and ignores the reference's
    `output_transform` keyword."""
    import os

    if gt_apd is None and annotations_folder is None:
        raise ValueError("get_apde_storer: give gt_apd or annotations_folder")

    def factory(output_transform=None, **kw):
        if gt_apd is not None:
            return metrics.APDEAccumulator(gt_apd, device)
        return metrics.APDEAccumulator.from_csv(os.path.join(annotations_folder, "mmapd_GT.csv"), device)

    return factory, lambda pred, **kwgs: metrics.apd(pred)


def get_cmd_storer(idx_to_class, mean_motion_per_class, if_consider_hip=False, device="cuda", **kwargs):
    """config_metrics.py:62-69 `get_cmd_storer` without ignite and without the dataset object: (a factory of
    `metrics.CMDAccumulator` over the dataset's `idx_to_class` / `mean_motion_per_class`, the
    `(motion_for_cmd(pred), class_idx)` transform of the evaluation dict).  `class_idx` (B,) are the batch's
    class indices (the reference looks them up from the metadata's class names).  Per batch:
    `acc.update(*transform(**out))`; at the end `acc.compute()`.  The factory takes and ignores the
    reference's `output_transform` keyword."""
    assert not if_consider_hip
    if len(idx_to_class) != len(mean_motion_per_class):
        raise ValueError(f"get_cmd_storer: {len(idx_to_class)} classes, {len(mean_motion_per_class)} mean motions")

    def factory(output_transform=None, **kw):
        return metrics.CMDAccumulator(mean_motion_per_class, device)

    return factory, lambda pred, class_idx, **kwgs: (metrics.motion_for_cmd(pred), class_idx)


class MetricSet:
    """What `metric_set` returns: `storers` maps every name of the result table to its accumulator."""

    def __init__(self, stats_funcs, storers, extra):
        self.stats_funcs, self.storers, self._extra = stats_funcs, storers, extra

    def update(self, pred=None, target=None, mm_gt=None, obs=None, class_idx=None, segment_idx=None, **kwargs) -> None:
        """One batch of the evaluation loop: pred (B, S, T, J, 3), target (B, T, J, 3), mm_gt the batch's
        multimodal ground truths, obs the observation, class_idx (B,) for CMD, segment_idx (optional) for
        APDE.  Everything is queued on the current stream."""
        out = dict(pred=pred, target=target, mm_gt=mm_gt, obs=obs, **kwargs)
        for name, fn in self.stats_funcs.items():
            self.storers[name].update(fn(**out))
        if "FID" in self._extra:
            self.storers["FID"].update(*self._extra["FID"](**out))
        if "CMD" in self._extra:
            self.storers["CMD"].update(*self._extra["CMD"](class_idx=class_idx, **out))
        if "APDE" in self._extra:
            self.storers["APDE"].update(self._extra["APDE"](**out), segment_idx)

    def all_reduce(self, group=None) -> "MetricSet":
        for s in self.storers.values():
            s.all_reduce(group)
        return self

    def compute(self) -> dict:
        """name -> Python float: one host copy per storer."""
        return {name: s.compute() for name, s in self.storers.items()}


def metric_set(stats_mode, skeleton_key, dataset_split="test", dataset_name="h36m", if_compute_cmd=False,
               if_compute_fid=False, if_compute_apde=False, device="cuda", **config) -> MetricSet:
    """config_metrics.py:71-96 `attach_engine_to_metrics` without ignite: one `metrics.MetricAccumulator` per
    `get_stats_funcs` entry ('max' where the name contains '_max', else 'avg'), FID for h36m + test +
    if_compute_fid (`get_fid_storer`: classifier_path / precomputed_folder), CMD for test + if_compute_cmd
    (`get_cmd_storer`: idx_to_class, mean_motion_per_class), APDE with if_compute_apde (`get_apde_storer`:
    gt_apd / annotations_folder).  `update(**batch)` per batch, `all_reduce()` across ranks, `compute()` the
    result table {name: float}."""
    stats = get_stats_funcs(stats_mode, skeleton_key, **config)
    storers = {k: metrics.MetricAccumulator("max" if "_max" in k else "avg") for k in stats}
    extra = {}
    if dataset_name == "h36m" and dataset_split == "test" and if_compute_fid:
        storers["FID"], extra["FID"] = get_fid_storer(device=device, **config)
    if dataset_split == "test" and if_compute_cmd:
        factory, extra["CMD"] = get_cmd_storer(device=device, **config)
        storers["CMD"] = factory()
    if if_compute_apde:
        factory, extra["APDE"] = get_apde_storer(device=device, **config)
        storers["APDE"] = factory()
    return MetricSet(stats, storers, extra)


class _LossAccumulator:
    """ignite.metrics.Loss: the batch-size-weighted mean of `loss_fn(y_pred, y)`; a float64 sum on the device of
    the losses, the row count on the host (shapes are known without a copy)."""

    def __init__(self, loss_fn):
        self.loss_fn, self.sum, self.count = loss_fn, None, 0

    def update(self, y_pred, y) -> None:
        with torch.no_grad():
            loss = self.loss_fn(y_pred, y)
        if loss.dim() != 0:
            raise ValueError("validation_set: loss_fn did not return the average loss")
        term = loss.detach().to(torch.float64) * y.shape[0]
        self.sum = term if self.sum is None else self.sum + term
        self.count += int(y.shape[0])

    def all_reduce(self, group=None):
        import torch.distributed as dist

        if self.sum is None:
            raise metrics.SkelDiffError("validation_set: Loss.all_reduce before any update on this rank")
        both = torch.stack([self.sum, torch.tensor(float(self.count), dtype=torch.float64, device=self.sum.device)])
        dist.all_reduce(both, op=dist.ReduceOp.SUM, group=group)
        self.sum, self.count = both[0], int(both[1])
        return self

    def compute(self) -> float:
        if self.sum is None:
            raise metrics.SkelDiffError("Loss must have at least one example before it can be computed.")
        return float(self.sum.cpu()) / self.count


class ValidationSet:
    """What `validation_set` returns: `storers` maps the accumulated names of the validation table to their state."""

    def __init__(self, kind, limbseq, loss_fn, device):
        self.kind, self.limbseq = kind, limbseq
        acc = partial(metrics.MetricAccumulator, "avg")
        self.storers = {"MPJPE": metrics.MPJPEAccumulator(device=device)}
        if kind == "autoencoder":
            self.storers.update(ADE=acc(), FDE=metrics.FDEAccumulator(device=device))
        else:
            self.storers.update(APD=acc(), ADE=acc(), LLVar=acc())
        if loss_fn is not None:
            self.storers["Loss"] = _LossAccumulator(loss_fn)

    def update(self, pred=None, target=None, pred_input=None, target_input=None, **kwargs) -> None:
        """One validation batch in metric space: target (B, T, J, 3); pred (B, T, J, 3) for the autoencoder, (B, S,
        T, J, 3) for the diffusion loop.  pred_input / target_input are the same pair in the model's input space,
        for the loss (the diffusion loop's loss is taken on the sample closest to target_input,
        train_utils.py:109).  Everything is queued on the current stream."""
        st = self.storers
        if self.kind == "autoencoder":
            st["MPJPE"].update(pred, target)
            st["ADE"].update(metrics.ade(pred=pred.unsqueeze(1), target=target))
            st["FDE"].update(pred, target)
        else:
            st["MPJPE"].update(pred, target, best=True)  # the best sample, read where it lies
            st["APD"].update(metrics.apd(pred=pred, target=target))
            st["ADE"].update(metrics.ade(pred=pred, target=target))
            st["LLVar"].update(metrics.limb_length_variance(pred=pred, limbseq=self.limbseq, mode="mean"))
        if "Loss" in st:
            if pred_input is None or target_input is None:
                raise ValueError("validation_set: built with a loss_fn, update needs pred_input and target_input")
            if self.kind == "diffusion":
                pred_input, target_input = metrics.choose_best_sample(pred_input, target_input)
            st["Loss"].update(pred_input, target_input)

    def all_reduce(self, group=None) -> "ValidationSet":
        for s in self.storers.values():
            s.all_reduce(group)
        return self

    def compute(self) -> dict:
        """The reference's `engine.state.metrics`: 'MPJPE' the time table (float64 host tensor), 'MPJPE_AVG' its
        mean (train_utils.py:70-73), the other names Python floats."""
        out = {}
        for name, s in self.storers.items():
            v = s.compute()
            out[name] = v if name == "MPJPE" else float(v)
            if name == "MPJPE":
                out["MPJPE_AVG"] = v.mean(0)
        return out


def validation_set(kind, skeleton_key, loss_fn=None, device="cuda") -> ValidationSet:
    """src/train_utils.py:56-95 `setup_validation_autoencoder` (kind 'autoencoder': MPJPE, MPJPE_AVG, ADE, FDE,
    Loss) and :97-137 `setup_validation_diffusion` (kind 'diffusion': MPJPE of the best sample, MPJPE_AVG, APD, ADE,
    LLVar, Loss) without ignite: `update(pred=, target=, pred_input=, target_input=)` per batch, `all_reduce()`
    across ranks, `compute()` the table.  `loss_fn(y_pred, y)` is the model's loss (omitted from the table when
    None).  No prediction is kept or copied to the host: the per-frame errors stream into float64 sums on the
    device (sd_frame_error_update), the limb-length variance is one read of pred (sd_limb_stats)."""
    if kind not in ("autoencoder", "diffusion"):
        raise ValueError(f"validation_set: kind {kind!r} not supported, expected 'autoencoder' or 'diffusion'")
    limbseq = skeletons.limbseq(skeleton_key) if kind == "diffusion" else None
    return ValidationSet(kind, limbseq, loss_fn, device)


__all__ = ["get_diffusion_latent_codes", "decode_latent_pred", "get_prediction", "process_evaluation_pair",
           "long_term_prediction_best_every50", "long_term_prediction_best_first50", "get_stats_funcs", "get_fid_storer",
           "get_apde_storer", "get_cmd_storer", "metric_set", "MetricSet", "validation_set", "ValidationSet"]
