"""Long-term rollouts and the prediction chain (skeletondiffusion_amd.evaluation) against the reference's
own src/eval_utils.py:44-99 outputs (tests/golden/longterm.npz, gen_golden_longterm.py): a stub
`get_prediction` returns seeded tables, so the rollouts only select, slice and concatenate and every
returned value and every recorded observation is compared exactly.  Then the real chain (HIP encoder,
sampler, decoder, selection) on a small H36M-shaped setup against the same calls written out here."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import build_release_diffusion, golden
from skeletondiffusion_amd import synthetic

# gen_golden_longterm.py: B sequences, S samples, OBS observed frames, PL frames per segment, J joints
B, S, OBS, PL, J = 3, 6, 4, 6, 5
FACTORS = {"f25": 2.5, "f2": 2}


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


def rollout_inputs(factor):
    """gen_golden_longterm.py:rollout_inputs restated: (data, target, table[segment])."""
    data, target = N((B, OBS, J, 3), 81), N((B, int(factor * PL), J, 3), 82)
    return data, target, [N((B, S, PL, J, 3), 90 + k) for k in range(math.ceil(factor))]


def stub_prediction(table, seen, first):
    """The generator's get_prediction: table[segment], (B * S, 1, ...) for best_first50's later
    segments; records the observation it was called with."""
    def get_prediction(obs, num_samples=S, extra=None):
        k = len(seen)
        seen.append(obs.clone())
        out = table[k]
        if first and k > 0:
            assert tuple(obs.shape) == (B * S, OBS, J, 3) and num_samples == 1
            out = out.reshape(B * S, 1, PL, J, 3)
        return out
    return get_prediction


def ref_rollout(first, data, target, table, factor):
    """float64 restatement of eval_utils.py:44-99 with the stub predictor: (target, pred, observations)."""
    n = math.ceil(factor)
    cut = int(factor * PL) % PL if int(factor) != factor else None
    obs, seen, preds = data, [], []
    for k in range(n):
        seen.append(obs.reshape(-1, *obs.shape[-3:]) if first and k > 0 else obs)
        pred = table[k]
        if k == n - 1 and cut is not None:
            pred = pred[:, :, :cut]
        if first:
            preds.append(pred)
            obs = pred[:, :, -OBS:]
        else:
            y = target[:, k * PL:(k + 1) * PL]
            d = (pred.double() - y.double().unsqueeze(1)).square().sum(-1).sqrt().mean(-1).mean(-1)
            best = pred[torch.arange(B), d.min(dim=-1).indices]
            preds.append(best)
            obs = best[:, -OBS:]
    pred = torch.cat(preds, dim=-3)
    return target, pred if first else pred.unsqueeze(1).repeat(1, S, 1, 1, 1), seen


CASES = [(fn, tag) for tag in FACTORS for fn in ("every", "first")]


def _check(z, key, target, pred, seen):
    assert np.array_equal(np.asarray(target.cpu()), z[f"{key}_target"])
    assert tuple(pred.shape) == z[f"{key}_pred"].shape and np.array_equal(np.asarray(pred.cpu()), z[f"{key}_pred"])
    assert len(seen) == sum(1 for k in z.files if k.startswith(f"{key}_obs"))
    for k, o in enumerate(seen):
        assert np.array_equal(np.asarray(o.cpu()), z[f"{key}_obs{k}"]), (key, k)


@pytest.mark.parametrize("fn,tag", CASES)
def test_restatement_matches_reference(fn, tag):
    data, target, table = rollout_inputs(FACTORS[tag])
    _check(golden("longterm"), f"{fn}_{tag}", *ref_rollout(fn == "first", data, target, table, FACTORS[tag]))


def test_module_surface():
    from skeletondiffusion_amd import evaluation as E

    for name in ("get_diffusion_latent_codes", "decode_latent_pred", "get_prediction",
                 "long_term_prediction_best_every50", "long_term_prediction_best_first50"):
        assert name in E.__all__ and callable(getattr(E, name))
    # the default process_evaluation_pair: the reference's shape assertion, then the inputs back
    pred, y, obs = torch.zeros(2, 3, 4, 5, 3), torch.zeros(2, 4, 5, 3), torch.zeros(2, 6, 5, 3)
    out = E.process_evaluation_pair(target=y, pred_dict={"pred": pred, "obs": obs})
    assert out[0] is y and out[1] is pred and out[2] is None and out[3] is obs
    with pytest.raises(AssertionError):
        E.process_evaluation_pair(target=y[:, :3], pred_dict={"pred": pred, "obs": obs})


# ---- device ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fn,tag", CASES)
def test_device_rollout_matches_reference(cuda, fn, tag):
    from skeletondiffusion_amd import evaluation as E

    factor = FACTORS[tag]
    data, target, table = rollout_inputs(factor)
    data, target, table = data.to(cuda), target.to(cuda), [t.to(cuda) for t in table]
    seen = []
    run = E.long_term_prediction_best_first50 if fn == "first" else E.long_term_prediction_best_every50
    tgt, pred, mm_gt, dat = run(data, target, None, stub_prediction(table, seen, fn == "first"),
                                E.process_evaluation_pair, S, {"long_term_factor": factor, "pred_length": PL})
    assert mm_gt is None and dat is data and pred.is_cuda and tgt.is_cuda
    _check(golden("longterm"), f"{fn}_{tag}", tgt, pred, seen)


@pytest.fixture(scope="module")
def h36m_model(cuda):
    """H36M J = 16 release Denoiser (T = 10) and a synthetic-weight AutoEncoder, as tools/eval_pipeline.py."""
    from skeletondiffusion_amd.core.network.autoencoder import AutoEncoder

    z = golden("release_h36m16_T10")
    d = build_release_diffusion(z, cuda)
    ae = AutoEncoder(node_types=torch.from_numpy(z["node_types"]), num_nodes=16, encoder_hidden_size=96,
                     decoder_hidden_size=96, latent_size=96, input_size=3, z_activation="tanh", enc_num_layers=1,
                     output_size=3, recurrent_arch_enc="StaticGraphGRU", recurrent_arch_decoder="StaticGraphGRU",
                     if_consider_hip=False).eval()
    synthetic.fill_module_(ae, 4321)
    return ae.to(cuda), d


E2E = dict(B=2, S=5, OBS=6, PH=8, SEED=7)


def _pipeline_calls(ae, d, obs, S, ph, seed):
    """The tools/eval_pipeline.py call sequence."""
    z_past = ae.get_past_embedding(obs)
    lat, _ = d.sample(batch_size=obs.shape[0] * S, x_cond=z_past, seed=seed)
    pred = ae.decode(obs.repeat_interleave(S, 0), lat, z_past.repeat_interleave(S, 0), ph=ph)
    return pred.view(obs.shape[0], S, ph, *obs.shape[2:])


@pytest.mark.gpu
def test_get_prediction_equals_pipeline_calls(cuda, h36m_model):
    from skeletondiffusion_amd import evaluation as E

    ae, d = h36m_model
    b, s, ph = E2E["B"], E2E["S"], E2E["PH"]
    obs = (N((b, E2E["OBS"], 16, 3), 51) * 0.3).to(cuda)
    want = _pipeline_calls(ae, d, obs, s, ph, E2E["SEED"])
    got = E.get_prediction(obs, model=(ae, d), num_samples=s, pred_length=ph, sampler_kwargs={"seed": E2E["SEED"]})
    assert got.shape == (b, s, ph, 16, 3) and torch.isfinite(got).all() and torch.equal(got, want)
    lat, z_past = E.get_diffusion_latent_codes(obs, (ae, d), num_samples=s, sampler_kwargs={"seed": E2E["SEED"]})
    assert lat.shape == (b * s, 16, 96) and z_past.shape == (b, 16, 96)
    assert torch.equal(E.decode_latent_pred(obs, lat, z_past, (ae, d), num_samples=s, pred_length=ph), want)


@pytest.mark.gpu
def test_rollout_end_to_end_equals_public_calls(cuda, h36m_model):
    """best_every50 over the real chain is bitwise the same chain written out from the public calls,
    with the reference's selection expression in CPU torch on the decoded futures.  (Synthetic weights
    make the five futures alike: on the MI355X the two smallest distances of a sequence differ by 3e-5
    to 9e-5 of their value, some 300 times float32's rounding of these means; the test prints them.)"""
    from skeletondiffusion_amd import evaluation as E

    ae, d = h36m_model
    b, s, n_obs, ph, factor = E2E["B"], E2E["S"], E2E["OBS"], E2E["PH"], 2
    obs = (N((b, n_obs, 16, 3), 51) * 0.3).to(cuda)
    target = (N((b, factor * ph, 16, 3), 52) * 0.3).to(cuda)
    predict = functools.partial(E.get_prediction, model=(ae, d), num_samples=s, pred_length=ph,
                                sampler_kwargs={"seed": E2E["SEED"]})
    tgt, pred, mm_gt, dat = E.long_term_prediction_best_every50(
        obs, target, None, predict, num_samples=s, config={"long_term_factor": factor, "pred_length": ph})
    assert torch.equal(tgt, target) and dat is obs and mm_gt is None and pred.shape == (b, s, factor * ph, 16, 3)

    cur, bests = obs, []
    for k in range(factor):
        out = _pipeline_calls(ae, d, cur, s, ph, E2E["SEED"]).cpu()
        y = target[:, k * ph:(k + 1) * ph].cpu()
        dist = torch.linalg.norm(out - y.unsqueeze(1), dim=-1).mean(-1).mean(-1)
        print("segment", k, "per-sample distances", dist.tolist())
        indeces = dist.min(axis=-1).indices
        best = out[torch.arange(b), indeces]
        bests.append(best)
        cur = best[..., -n_obs:, :, :].to(cuda)
    want = torch.cat(bests, dim=-3).unsqueeze(1).repeat(1, s, 1, 1, 1)
    assert torch.equal(pred.cpu(), want)
