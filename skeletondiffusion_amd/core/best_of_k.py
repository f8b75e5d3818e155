"""The reference Trainer's best-of-k training relaxation (src/core/trainer.py:182-244) on the device.

`train_pick_best_sample_among_k = k > 1`: `NonisotropicGaussianDiffusion.forward(data, x_cond,
n_train_samples=k)` draws k noisy copies of every training sequence (p_losses' repeat_interleave,
base.py:264-268), and the loss of each sequence is the diffusion loss of the copy whose sample is
closest to the ground truth in `similarity_space`:
  latent_space -- the diffusion loss itself;
  input_space  -- AutoEncoder.loss(reduction='none') of the decoded samples against the future
                  (`sd_gru_decode` + `sd_pose_loss`);
  metric_space -- the ADE of the decoded samples in metric space (`sd_ade_fde` per_sample_ade).
The Trainer itself (ignite engine, EMA, optimiser loop) stays out of scope; these are
its three methods as functions of the state they read, with the reference's signatures, shapes and
return values.  Every step after `model(...)` runs on HIP kernels: the Mahalanobis loss
(training.MahalanobisLossFunction), the decoder, the similarity and the selection with its
gradient (training.BestOfKFunction).
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import nn

from .. import metrics as _metrics
from .. import training as _training
from .diffusion.base import LatentDiffusion, extract

SPACES = ("input_space", "metric_space", "latent_space")


def decode_diffusion_sample(samples, obs, autoencoder, x_cond=None, prediction_horizon=None):
    """trainer.py:278-287: decode the (b * k) sampled latents from each sequence's observed past
    (repeated k times) -> (out (b, k, ph, J, F), samples (b, k, J, D))."""
    x_t = obs.repeat_interleave(samples.shape[0] // obs.shape[0], dim=0)
    out = autoencoder.decode(x_t, samples, x_cond, prediction_horizon)
    out = out.view(obs.shape[0], -1, *out.shape[1:])
    return out, samples.view(obs.shape[0], -1, *samples.shape[1:])


def to_comparison_space_train(samples, diff_input, past_seq, autoencoder, fut_seq, space="latent_space", x_cond=None,
                              prediction_horizon=None, transform_to_metric_space: Optional[Callable] = None):
    """trainer.py:182-205 -> (out_comparespace, fut_seq_comparespace) of equal shape."""
    assert space in SPACES, f"Similarity space must be one of {SPACES} but is {space}"
    num_samples = samples.shape[0] // past_seq.shape[0]
    if x_cond is not None:
        x_cond = x_cond.repeat_interleave(num_samples, dim=0)
    if space in ("input_space", "metric_space"):
        ph = prediction_horizon if prediction_horizon is not None else fut_seq.shape[1]
        out, _ = decode_diffusion_sample(samples, past_seq, autoencoder, x_cond=x_cond, prediction_horizon=ph)
    if space == "input_space":
        out_c = out
        fut_c = fut_seq.unsqueeze(1).repeat_interleave(num_samples, dim=1)
    elif space == "metric_space":
        if transform_to_metric_space is None:
            raise ValueError("metric_space needs the skeleton's transform_to_metric_space")
        out_c = transform_to_metric_space(out).flatten(start_dim=3)
        fut_c = transform_to_metric_space(fut_seq).unsqueeze(1).flatten(start_dim=3).repeat_interleave(num_samples,
                                                                                                         dim=1)
    else:
        out_c = samples.view(diff_input.shape[0], -1, *samples.shape[1:])
        fut_c = diff_input.unsqueeze(1).repeat_interleave(num_samples, dim=1)
    assert out_c.shape == fut_c.shape
    return out_c, fut_c


def get_ksimilarity_loss(diffusion_loss, out_comparespace, fut_seq_comparespace, similarity_space="latent_space",
                         autoencoder=None, **kwargs):
    """trainer.py:207-222 -> (loss (b,), closest2gt_idx (b,)).  The similarity target is one future
    per sequence (the reference repeats it k times; the first copy is read)."""
    assert similarity_space in SPACES, f"Similarity space must be one of {SPACES} but is {similarity_space}"
    b = out_comparespace.shape[0]
    k = diffusion_loss.numel() // b
    with torch.no_grad():
        if similarity_space == "input_space":
            mse = autoencoder.loss_pose_type == "mse"
            assert mse or autoencoder.loss_pose_type in ("l1", "L1"), "Not implemnted"
            sim = _training.pose_loss(out_comparespace, fut_seq_comparespace[:, 0], mse)
        elif similarity_space == "metric_space":
            # ||out - fut|| over the flattened (J * 3) features, mean over frames: the per-sample ADE
            sim = _metrics.ade(fut_seq_comparespace[:, 0], out_comparespace, reduction="none")
        else:
            sim = None  # the diffusion loss itself
    loss, idx = _training.best_of_k(diffusion_loss.reshape(-1), k, sim)
    assert len(loss.shape) == 1 and loss.shape[0] == b
    return loss, idx


def _refuse_unselectable(model) -> None:
    """The selected-row step runs the Denoiser twice on the same rows: anything random inside the
    forward would have to be shared by both passes, so it is refused by name."""
    if getattr(model, "self_condition", False):
        raise ValueError("pick_best_loss_selected: self_condition=True is not supported (the coin flip of p_losses "
                         "would have to be shared by the scoring and the selected pass)")
    for name, m in model.named_modules():
        if isinstance(m, nn.Dropout) and m.p > 0 and m.training:
            raise ValueError(f"pick_best_loss_selected: Dropout {name!r} has p = {m.p} in training mode (the scoring "
                             "and the selected pass would drop different units)")


def _q_sample_rows(model, data, t, k, sel, noise, seed, step, row0, hip):
    """x_t and its noise for all b k rows (sel None: repeat_interleave order) or for the copy
    sel[s] of each sequence -> (x_t, eps, x_start rows, t rows).  On the HIP path a shape outside
    sd_q_sample_groups' limits (J <= 64, D % 4 == 0, D <= 256) raises SkelDiffError naming the
    argument; there is no fall-back to the torch ops."""
    b = data.shape[0]
    if sel is None:
        x0r = data.repeat_interleave(k, dim=0) if k > 1 else data
        tr = t.repeat_interleave(k, dim=0) if k > 1 else t
    else:
        x0r, tr = data, t
    if hip:
        from .diffusion import IsotropicGaussianDiffusion, NonisotropicGaussianDiffusion
        q = type(model).q_sample
        if q is NonisotropicGaussianDiffusion.q_sample:
            tables = dict(M=model.Umm_sqrt_Lambda_bar_t)
        elif q is IsotropicGaussianDiffusion.q_sample:
            tables = dict(sqrt_one_minus_alphas_cumprod=model.sqrt_one_minus_alphas_cumprod)
        else:
            raise NotImplementedError(f"pick_best_loss_selected: {type(model).__name__}.q_sample is not one the HIP "
                                      "forward process covers (nonisotropic, isotropic)")
        x, eps = _training.q_sample_groups(data, t, model.sqrt_alphas_cumprod, k, sel=sel, noise=noise, seed=seed,
                                           step=step, row0=row0, return_noise=True, **tables)
        return x, eps, x0r, tr
    eps = noise if sel is None else noise.index_select(0, torch.arange(b, device=data.device) * k + sel)
    return model.q_sample(x_start=x0r, t=tr, noise=eps), eps, x0r, tr


def _loss_rows(model, x, eps, x0r, tr, x_cond):
    """feed_model + the objective's target + loss_rows, as p_losses (base.py:270-298) -> (loss, model_out)."""
    out = model.feed_model(x, tr, x_self_cond=None, x_cond=x_cond)
    if model.objective == "pred_noise":
        target = eps
    elif model.objective == "pred_x0":
        target = x0r
    elif model.objective == "pred_v":
        target = model.predict_v(x0r, tr, eps)
    else:
        raise ValueError(f"unknown objective {model.objective}")
    return model.loss_rows(out, target, tr), out


def _selected_passes(model, data, x_cond, k: int, similarity_space="latent_space", autoencoder=None, past_seq=None,
                     fut_seq=None, prediction_horizon=None, transform_to_metric_space=None, t=None, noise=None,
                     seed=None, step=0, row0=0, mark: Optional[Callable[[str], None]] = None):
    """The body of `pick_best_loss_selected`, not part of the interface -> (loss, closest2gt_idx, the
    selected pass's loss rows (b,), the scoring pass's loss rows (b k,) or None when k == 1): the tests
    compare the two sets of rows.  `mark(name)` is called after each phase ('scoring_forward', 'decode',
    'selection', 'selected_forward'): tools/bench_best_of_k.py records a device event there."""
    assert similarity_space in SPACES, f"Similarity space must be one of {SPACES} but is {similarity_space}"
    _refuse_unselectable(model)
    if k < 1:
        raise ValueError("pick_best_loss_selected: k must be >= 1")
    b = data.shape[0]
    if noise is not None and tuple(noise.shape) != (b * k, *data.shape[1:]):
        raise ValueError(f"pick_best_loss_selected: noise must have shape {(b * k, *data.shape[1:])} "
                         f"(b * k rows in repeat_interleave order), got {tuple(noise.shape)}")
    mark = mark or (lambda name: None)
    if t is None:
        t = torch.randint(0, model.num_timesteps, (b,), device=data.device).long()
    hip = data.is_cuda and data.dtype == torch.float32 and _training.hip_training_enabled()
    # the Philox stream stands for the library's own white noise only: a model that overrides
    # get_white_noise / get_noise keeps its noise, as under p_losses, drawn once for all b k rows
    own_noise = (type(model).get_white_noise is not LatentDiffusion.get_white_noise
                 or type(model).get_noise is not LatentDiffusion.get_noise)
    if noise is None and (own_noise or not hip):
        noise = model.get_white_noise(data.repeat_interleave(k, dim=0) if k > 1 else data,
                                      t.repeat_interleave(k, dim=0) if k > 1 else t)
        if tuple(noise.shape) != (b * k, *data.shape[1:]):
            raise ValueError(f"pick_best_loss_selected: {type(model).__name__}.get_white_noise returned shape "
                             f"{tuple(noise.shape)}, not {(b * k, *data.shape[1:])}")
    if seed is None:  # a host draw (torch.manual_seed controls it); unused when the noise is supplied
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0
    q_args = (noise, seed, step, row0, hip)

    idx, rows_all = None, None
    if k > 1:
        with torch.no_grad(), _training.hip_forward_only():
            x, eps, x0r, tr = _q_sample_rows(model, data, t, k, None, *q_args)
            rows_all, samples = _loss_rows(model, x, eps, x0r, tr, x_cond)
            mark("scoring_forward")
            sim = out_c = fut_c = None  # latent_space: the diffusion loss itself
            if similarity_space != "latent_space":
                out_c, fut_c = to_comparison_space_train(samples, diff_input=data, past_seq=past_seq,
                                                         autoencoder=autoencoder, fut_seq=fut_seq,
                                                         space=similarity_space, x_cond=x_cond,
                                                         prediction_horizon=prediction_horizon,
                                                         transform_to_metric_space=transform_to_metric_space)
                mark("decode")
                if similarity_space == "input_space":
                    mse = autoencoder.loss_pose_type == "mse"
                    assert mse or autoencoder.loss_pose_type in ("l1", "L1"), "Not implemnted"
                    sim = _training.pose_loss(out_c, fut_c[:, 0], mse)
                else:
                    sim = _metrics.ade(fut_c[:, 0], out_c, reduction="none")
            else:
                mark("decode")
            if hip:
                _, idx = _training.best_of_k(rows_all.reshape(-1), k, sim)
            else:
                idx = (rows_all if sim is None else sim).reshape(b, k).min(dim=-1).indices
            # nothing of b k rows outlives the scoring pass but its loss rows (returned for the tests)
            del x, eps, x0r, tr, samples, out_c, fut_c, sim
        mark("selection")
    x, eps, x0r, tr = _q_sample_rows(model, data, t, k, idx, *q_args)
    rows_sel, _ = _loss_rows(model, x, eps, x0r, tr, x_cond)
    loss = (rows_sel * extract(model.loss_weight, t, rows_sel.shape)).mean()
    mark("selected_forward")
    return loss, idx, rows_sel, rows_all


def pick_best_loss_selected(model, data, x_cond, k: int, similarity_space="latent_space", autoencoder=None,
                            past_seq=None, fut_seq=None, prediction_horizon=None, transform_to_metric_space=None,
                            t=None, noise=None, seed=None, step=0, row0=0):
    """`pick_best_loss` with only the chosen copy of each sequence under autograd.
    Rows are independent in the Denoiser (mixing and attention are over joints, the norms per row), so:
      scoring pass   no_grad + training.hip_forward_only(): q_sample over all b k rows, feed_model,
                     loss_rows, the similarity in `similarity_space`, sd_best_of_k -> closest2gt_idx;
      selected pass  with autograd: q_sample of the b chosen rows, regenerated bit for bit from
                     (seed, step, row0 + row) or read from `noise`, feed_model, loss_rows, then
                     (loss * loss_weight[t]).mean().
    The parameter gradients equal pick_best_loss's up to the summation order of the weight-gradient
    reductions, with the activations of b rows kept instead of b k.  Returns (loss, closest2gt_idx);
    k == 1 runs the selected pass only and returns (loss, None).
    `t` (b,) defaults to torch.randint as in forward(); `noise` (b k, J, D) is the supplied noise in
    repeat_interleave order, otherwise the draws are the device Philox stream keyed (seed, step,
    row0 + row) (`seed` None: drawn on the host from torch's global RNG).  Nothing here synchronises
    with the host: closest2gt_idx stays on the device.
    On the CPU, or with set_hip_training(False), the same two passes run on torch ops with the supplied
    noise or the model's get_white_noise (torch.randn); input_space / metric_space need the HIP decoder
    and raise without it.  A model that overrides get_white_noise / get_noise gets its own noise on
    every path, as under p_losses: it is drawn once for all b k rows and read by both passes, so the
    Philox arguments are unused and b k rows of noise are kept.
    On the HIP path the forward process is sd_q_sample_groups and nothing else: a q_sample other than
    the nonisotropic / isotropic one raises NotImplementedError, a shape outside the kernel's limits
    (J <= 64, D % 4 == 0, D <= 256) raises SkelDiffError naming the argument.
    Refused by name: self_condition=True, a Dropout with p > 0 in training mode, a noise of another shape."""
    loss, idx, _, _ = _selected_passes(model, data, x_cond, k, similarity_space=similarity_space,
                                       autoencoder=autoencoder, past_seq=past_seq, fut_seq=fut_seq,
                                       prediction_horizon=prediction_horizon,
                                       transform_to_metric_space=transform_to_metric_space, t=t, noise=noise,
                                       seed=seed, step=step, row0=row0)
    return loss, idx


def pick_best_loss(model, data, x_cond, k: int, similarity_space="latent_space", autoencoder=None, past_seq=None,
                   fut_seq=None, prediction_horizon=None, transform_to_metric_space=None):
    """Trainer.loss (trainer.py:224-234) with train_pick_best_sample_among_k = k: the scalar the
    optimiser steps on.  Returns (loss, closest2gt_idx or None)."""
    loss, diff_weights, samples = model(data, x_cond=x_cond, n_train_samples=k)
    idx = None
    if k > 1:
        out_c, fut_c = to_comparison_space_train(samples, diff_input=data, past_seq=past_seq, autoencoder=autoencoder,
                                                 fut_seq=fut_seq, space=similarity_space, x_cond=x_cond,
                                                 prediction_horizon=prediction_horizon,
                                                 transform_to_metric_space=transform_to_metric_space)
        sim_loss, idx = get_ksimilarity_loss(loss, out_c, fut_c, similarity_space=similarity_space,
                                             autoencoder=autoencoder)
    else:
        sim_loss = loss
    return (sim_loss * diff_weights).mean(), idx
