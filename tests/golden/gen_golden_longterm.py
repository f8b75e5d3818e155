#!/usr/bin/env python3
"""Generate tests/golden/longterm.npz by running the REFERENCE's own best-sample selection, mpjpe and
long-term rollouts on the CPU (src/metrics/utils.py:12-30 choose_best_sample / get_best_sample_idx,
src/metrics/multimodal.py:37-42 mpjpe, src/eval_utils.py:44-99 long_term_prediction_best_every50 /
_best_first50).

Build-container tool only, like gen_golden_realism.py: it imports the read-only reference tree (which
does not exist on the GPU box) and no test uses it.  Only reference outputs are written; the inputs are
regenerated from their seeds by the consumers (tests/test_best_sample.py:selection_inputs and
tests/test_longterm.py:rollout_inputs restate the recipes below).

Selection cases.  The reference's functions run on the float32 inputs in float32 and in float64
(`.double()`); the float64 values are stored.  The per-sample distances are the reference's `mpjpe` of
each sample on its own.  Two conditions make the index a fact of the inputs and not of rounding, and
both are asserted here: the two smallest distances of a sequence differ by more than 1e-3 of their
value (except where two samples are byte copies: the tie), and the float32 and float64 runs pick the
same index.

Rollout cases.  `get_prediction` is a stub that returns table[segment] (seeded tensors: the rollouts
then only select, slice and concatenate) and records the `obs` it was called with;
`process_evaluation_pair` is the identity after the reference's shape assertion
(eval_prepare_model.py:131-134), and also asserts the 1e-3 gap for the segment's selection.

`src.eval_utils` calls `math.ceil` without importing `math`: the module gets the attribute here.
`src.metrics.cmd` (pulled in by `src.metrics`) imports `ignite`, absent here: the same empty stub as
gen_golden_realism.py is registered first.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_longterm.py
"""
from __future__ import annotations

import math
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SKELDIFF_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

from skeletondiffusion_amd import synthetic  # noqa: E402


def _install_ignite_stub() -> None:
    pkg, met, exc = (types.ModuleType(n) for n in ("ignite", "ignite.metrics", "ignite.exceptions"))
    met.Metric = type("Metric", (), {})
    exc.NotComputableError = type("NotComputableError", (RuntimeError,), {})
    pkg.metrics, pkg.exceptions = met, exc
    sys.modules.update({"ignite": pkg, "ignite.metrics": met, "ignite.exceptions": exc})


_install_ignite_stub()
sys.path.insert(0, REF)
import src.eval_utils as EU  # noqa: E402
from src.metrics.multimodal import mpjpe  # noqa: E402
from src.metrics.utils import choose_best_sample, get_best_sample_idx  # noqa: E402

EU.math = math
torch.set_num_threads(8)

GAP = 1e-3


def N(shape, seed):
    return torch.from_numpy(synthetic.normal(shape, seed=seed))


# name -> ((B, S, T, J, 3), pred seed, target seed)
SELECTION_CASES = {
    "tie": ((3, 5, 7, 4, 3), 71, 72),       # samples 1 and 3 of sequence 1: byte copies, and the closest
    "s50": ((2, 50, 20, 16, 3), 73, 74),
    "amass": ((2, 3, 120, 21, 3), 75, 76),  # the AMASS future: 2,520 joints per sample
    "s64": ((1, 64, 1, 17, 3), 77, 78),     # the sample limit; 51 floats per sample
    "mano": ((2, 1, 5, 51, 3), 79, 80),
}


def selection_inputs(name):
    shape, sp, st = SELECTION_CASES[name]
    pred, target = N(shape, sp), N(shape[:1] + shape[2:], st)
    if name == "tie":  # sequence 1: sample 1 moved halfway to the target (the closest), sample 3 its copy
        pred[1, 1] = 0.5 * (pred[1, 1] + target[1])
        pred[1, 3] = pred[1, 1]
    return pred, target


def assert_gap(dist, ties=()):
    """dist (B, S) float64: the two smallest of every sequence differ by more than GAP of their value."""
    for b in range(dist.shape[0]):
        if dist.shape[1] < 2 or b in ties:
            continue
        lo = np.sort(dist[b])[:2]
        assert lo[1] - lo[0] > GAP * lo[1], (b, lo)


def selection(arrays):
    for name in SELECTION_CASES:
        pred, target = selection_inputs(name)
        res = {}
        for tag, (p, t) in (("f32", (pred, target)), ("f64", (pred.double(), target.double()))):
            best, mask = get_best_sample_idx(p, t)
            best2, y = choose_best_sample(p, t)
            assert torch.equal(best, best2) and y is t
            per = torch.stack([mpjpe(t, p[:, s:s + 1]) for s in range(p.shape[1])], 1)
            res[tag] = (mpjpe(t, p).numpy(), per.numpy(), mask.long().argmax(1).numpy(), best.numpy())
        (m32, d32, i32, b32), (m64, d64, i64, b64) = res["f32"], res["f64"]
        assert np.array_equal(i32, i64), (name, i32, i64)
        assert np.array_equal(b32.astype(np.float64), b64)
        assert np.array_equal(d64.min(1), m64)
        assert_gap(d64, ties=(1,) if name == "tie" else ())
        if name == "tie":
            assert d64[1, 1] == d64[1, 3] == d64[1].min() and i64[1] == 1  # the lower index wins
        arrays[f"{name}_mpjpe"], arrays[f"{name}_dist"] = m64, d64
        arrays[f"{name}_idx"], arrays[f"{name}_best"] = i64.astype(np.int64), b32
        print(f"  {name:6s} idx {i64.tolist()}  f32-vs-f64 distance, max relative: "
              f"{float(np.max(np.abs(d32 - d64) / d64)):.2e}")


# rollout shape: B sequences, S samples, OBS observed frames, PL frames per segment, J joints
B, S, OBS, PL, J = 3, 6, 4, 6, 5
ROLLOUT_SEEDS = {"data": 81, "target": 82, "table": 90}  # table[segment]: seed 90 + segment
FACTORS = {"f25": 2.5, "f2": 2}


def rollout_inputs(factor):
    data, target = N((B, OBS, J, 3), ROLLOUT_SEEDS["data"]), N((B, int(factor * PL), J, 3), ROLLOUT_SEEDS["target"])
    table = [N((B, S, PL, J, 3), ROLLOUT_SEEDS["table"] + k) for k in range(math.ceil(factor))]
    return data, target, table


def identity_pair(target, pred_dict):
    pred, obs = pred_dict["pred"], pred_dict["obs"]
    batch_size, n_samples, seq_length, num_joints, features = pred.shape
    assert features == 3 and list(target.shape) == [batch_size, seq_length, num_joints, features]
    d = torch.linalg.norm(pred.double() - target.double().unsqueeze(1), dim=-1).mean(-1).mean(-1)
    assert_gap(d.numpy())
    return target, pred, None, obs


def rollouts(arrays):
    for tag, factor in FACTORS.items():
        for fn_name, fn in (("every", EU.long_term_prediction_best_every50),
                            ("first", EU.long_term_prediction_best_first50)):
            data, target, table = rollout_inputs(factor)
            seen = []

            def get_prediction(obs, num_samples=S, extra=None):
                k = len(seen)
                seen.append(obs.clone())
                out = table[k]
                if fn_name == "first" and k > 0:  # B * S rows, one sample each
                    assert tuple(obs.shape) == (B * S, OBS, J, 3) and num_samples == 1
                    out = out.reshape(B * S, 1, PL, J, 3)
                return out

            tgt, pred, mm_gt, dat = fn(data, target, None, get_prediction, identity_pair, S,
                                       {"long_term_factor": factor, "pred_length": PL})
            assert mm_gt is None and torch.equal(dat, data) and len(seen) == math.ceil(factor)
            assert tuple(pred.shape) == (B, S, int(factor * PL), J, 3) and torch.equal(tgt, target)
            key = f"{fn_name}_{tag}"
            arrays[f"{key}_target"], arrays[f"{key}_pred"] = tgt.numpy(), pred.contiguous().numpy()
            for k, o in enumerate(seen):
                arrays[f"{key}_obs{k}"] = o.numpy()
            print(f"  {key}: pred {tuple(pred.shape)}, {len(seen)} segments")


def main():
    arrays = {}
    print("selection cases:")
    selection(arrays)
    print("rollout cases:")
    rollouts(arrays)
    path = os.path.join(HERE, "longterm.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
