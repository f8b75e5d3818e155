#!/usr/bin/env python3
"""Generate tests/golden/fid.npz by running the REFERENCE's own FID classifier and fid() on the CPU
(src/metrics/fid_classifier.py:ClassifierForFID.get_fid_features, src/metrics/fid.py:fid).

Build-container tool only, like gen_golden_realism.py: it imports the read-only reference tree and no
test uses it.  Only reference outputs are written: the float32 activations and the fid() values.  The
weights, inputs and initial hidden states are regenerated from their seeds by the consumers
(tests/test_fid.py restates the recipe below).

Weights.  Every parameter of ClassifierForFID(input_size=3 J), in sorted name order i = 0, 1, ..., is
synthetic.uniform(shape, seed=100 + i, low=-0.15, high=0.15).  At that bound the activations are
unsaturated (per-feature std 0.10-0.17, max |a| below 1); at +-0.3 they saturate to +-1.000, which would
hide kernel errors, and torch's default init leaves them at std 0.02.

`fid.py` imports `ignite` (absent here: an empty stub is registered first) and `scipy` (needed: fid()
calls scipy.linalg.sqrtm).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_fid.py
"""
from __future__ import annotations

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
from src.metrics.fid import fid  # noqa: E402
from src.metrics.fid_classifier import ClassifierForFID  # noqa: E402

torch.set_num_threads(8)

# name -> ((B, S, T, J), whether fid() is stored)
CASES = {
    "long": ((2, 3, 100, 16), False),   # the release length; the reference forgets h0 to 1e-7 here
    "short": ((40, 2, 7, 16), True),    # h0 decides the result
    "one": ((33, 2, 1, 16), True),      # one frame, no recurrence
    "j15": ((5, 3, 4, 15), False),      # input_size 45, through a padded K
}


def classifier(J):
    m = ClassifierForFID(input_size=3 * J, hidden_size=128, hidden_layer=2, output_size=15, device="cpu")
    with torch.no_grad():
        for i, (name, p) in enumerate(sorted(m.named_parameters(), key=lambda kv: kv[0])):
            p.copy_(torch.from_numpy(synthetic.uniform(tuple(p.shape), seed=100 + i, low=-0.15, high=0.15)))
    return m.eval()


def inputs(B, S, T, J):
    pred = 0.4 * torch.from_numpy(synthetic.normal((B, S, T, J, 3), 11))
    target = 0.4 * torch.from_numpy(synthetic.normal((B, T, J, 3), 12))
    h_pred = torch.from_numpy(synthetic.normal((2, B * S, 128), 13))
    h_gt = torch.from_numpy(synthetic.normal((2, B, 128), 14))
    return pred, target, h_pred, h_gt


def storer_layout(pred, target):
    """fid.py:111-117: what MetricStorerFID.update hands to get_fid_features."""
    pred_ = pred.reshape(*pred.shape[:-2], -1)
    pred_ = pred_.reshape(-1, *pred_.shape[2:]).permute(0, 2, 1)
    target_ = target.reshape(*target.shape[:-2], -1).permute(0, 2, 1)
    return pred_, target_


def main():
    arrays = {}
    for name, ((B, S, T, J), with_fid) in CASES.items():
        m = classifier(J)
        pred, target, h_pred, h_gt = inputs(B, S, T, J)
        pred_, target_ = storer_layout(pred, target)
        with torch.no_grad():
            ap = m.get_fid_features(motion_sequence=pred_.float(), hidden_unit=h_pred).cpu().data.numpy()
            ag = m.get_fid_features(motion_sequence=target_.float(), hidden_unit=h_gt).cpu().data.numpy()
            m64 = classifier(J).double()
            # (get_fid_features casts its input to float; the float64 run calls the same layers)
            def f64(x, h):
                o, _ = m64.recurrent(x.permute(2, 0, 1).contiguous().double(), h.double())
                return torch.tanh(m64.linear1(o[-1])).numpy()
            dp, dg = np.abs(ap - f64(pred_, h_pred)).max(), np.abs(ag - f64(target_, h_gt)).max()
            zero = m.get_fid_features(motion_sequence=pred_.float(), hidden_unit=torch.zeros_like(h_pred)).numpy()
        assert ap.dtype == np.float32 and ap.shape == (B * S, 30) and ag.shape == (B, 30)
        arrays[f"{name}_pred_act"], arrays[f"{name}_gt_act"] = ap, ag
        line = (f"{name:6s} (B, S, T, J) = {(B, S, T, J)}: reference float32 vs float64 {max(dp, dg):.2e}; "
                f"max |a| {np.abs(ap).max():.3f}, per-feature std {ap.std(0).min():.3f}-{ap.std(0).max():.3f}; "
                f"h0 moves the features by {np.abs(ap - zero).max():.1e}")
        if with_fid:
            v = fid(ag, ap)  # fid.py:128: (gt activations, pred activations)
            assert np.isfinite(v)
            arrays[f"{name}_fid"] = np.float64(v)
            line += f"; fid {v:.6f}"
        print(line)
    path = os.path.join(HERE, "fid.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
