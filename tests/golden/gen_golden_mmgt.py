#!/usr/bin/env python3
"""Generate tests/golden/mmgt.npz by running the REFERENCE's own multimodal-ground-truth search, apd and APDE
storer on the CPU (src/data/loaders/base/math_utils.py:get_multimodal_gt, src/metrics/multimodal.py:apd,
src/metrics/apde.py:MetricStorerAPDE).

Build-container tool only, like gen_golden_fid.py: it imports the read-only reference tree and no test uses it.
The reference modules are loaded by file (their packages import the whole data pipeline); `apde.py` imports
`ignite` (absent here: a stub Metric whose constructor calls reset(), as ignite's does, is registered first),
`pandas` and, for math_utils, `tqdm` (both needed).

Stored:
  obs (150, 2, 16, 3) f32   torch.manual_seed(0); the last frame is one of 10 centres randn * 0.3 (segment i in
                            cluster i % 10) plus randn * 0.05, drawn in the order centres, jitter, obs; thr = 0.5
  row_ptr, col              the reference's get_multimodal_gt dict as CSR: a stub loader of batch size 64 (3 batches,
                            the last ragged), identity transform_to_metric_space, ordered segment_idx
  futures (150, 20, 16, 3) f32, gt_apd (150,) f64   the reference apd(futures[set_i][None]) in float64; every set has
                            at most 25 members, where torch.cdist forms differences (checked against the
                            direct expression below)
  csv_gt_apd (150,) f64     gt_apd with a handful of entries set to 0, as written to the temporary mmapd_GT.csv
  apd_pred (150,) f32, apde f64   the reference MetricStorerAPDE fed that CSV and apd_pred in batches of 64, 64, 22

The band condition: no pair has |d64 - thr| <= 4 D 2^-24 thr (d64 the float64 distance, D = 48), the worst-case
float32 summation error of any order, so a float32 implementation in any order finds the same hits.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mmgt.py
"""
from __future__ import annotations

import csv
import importlib.util
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SKELDIFF_REFERENCE", "/root/reference")

N, J, CLUSTERS, THR, BATCH = 150, 16, 10, 0.5, 64


def _install_ignite_stub() -> None:
    class Metric:
        def __init__(self, output_transform=lambda x: x, **kwargs):
            self._output_transform = output_transform
            self.reset()

        def reset(self):
            pass

    pkg, met, exc = (types.ModuleType(n) for n in ("ignite", "ignite.metrics", "ignite.exceptions"))
    met.Metric = Metric
    exc.NotComputableError = type("NotComputableError", (RuntimeError,), {})
    pkg.metrics, pkg.exceptions = met, exc
    sys.modules.update({"ignite": pkg, "ignite.metrics": met, "ignite.exceptions": exc})


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_install_ignite_stub()
if not hasattr(np, "NaN"):  # apde.py:18 spells it the NumPy 1 way
    np.NaN = np.nan
math_utils = _load("ref_math_utils", "src/data/loaders/base/math_utils.py")
multimodal = _load("ref_multimodal", "src/metrics/multimodal.py")
apde_mod = _load("ref_apde", "src/metrics/apde.py")

torch.set_num_threads(8)


class _Loader:
    """What get_multimodal_gt reads of a DataLoader: batch_size, dataset (len, skeleton), len and iteration."""

    def __init__(self, obs, batch_size):
        self.obs, self.batch_size = obs, batch_size
        skeleton = types.SimpleNamespace(transform_to_metric_space=lambda x: x)
        self.dataset = type("D", (), {"skeleton": skeleton, "__len__": lambda s: obs.shape[0]})()

    def __len__(self):
        return (self.obs.shape[0] + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for a in range(0, self.obs.shape[0], self.batch_size):
            b = min(a + self.batch_size, self.obs.shape[0])
            yield self.obs[a:b], None, {"segment_idx": torch.arange(a, b)}


def main():
    torch.manual_seed(0)
    centres = torch.randn(CLUSTERS, J, 3) * 0.3
    jitter = torch.randn(N, J, 3) * 0.05
    obs = torch.randn(N, 2, J, 3)
    obs[:, -1] = centres[torch.arange(N) % CLUSTERS] + jitter
    futures = torch.randn(N, 20, J, 3)
    apd_noise = torch.randn(N)

    mmgt = math_utils.get_multimodal_gt(_Loader(obs, BATCH), THR, recover_landmarks=True)
    assert sorted(mmgt) == list(range(N))
    sizes = [len(mmgt[i]) for i in range(N)]
    row_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    col = np.array([c for i in range(N) for c in sorted(mmgt[i])], dtype=np.int64)

    # the band condition, on float64 distances formed from differences
    x = obs[:, -1].reshape(N, -1).double()
    d64 = ((x[:, None] - x[None]) ** 2).sum(-1).sqrt()
    D = x.shape[1]
    band = 4 * D * 2.0 ** -24 * THR
    gap = float((d64 - THR).abs().min())
    assert gap > band, f"a pair lies within {band:.2e} of the threshold ({gap:.2e}): choose another seed"
    hits64 = (d64 < THR).nonzero()
    assert hits64.shape[0] == len(col) and (hits64[:, 1].numpy() == col).all(), "the reference's hits are not the float64 ones"
    print(f"{len(col)} hits, set sizes {min(sizes)}..{max(sizes)}, smallest |d - thr| {gap:.2e} = {gap / band:.0f} x the band {band:.2e}")

    assert max(sizes) <= 25  # above, torch.cdist's default mode switches to the matmul form
    gt_apd = np.zeros(N)
    for i in range(N):
        members = torch.tensor(sorted(mmgt[i]))
        f = futures[members].double()
        gt_apd[i] = float(multimodal.apd(f[None])[0])
        if len(members) > 1:
            flat = f.reshape(len(members), -1)
            dd = ((flat[:, None] - flat[None]) ** 2).sum(-1).sqrt()
            iu = torch.triu_indices(len(members), len(members), offset=1)
            direct = float(dd[iu[0], iu[1]].mean())
            assert abs(direct - gt_apd[i]) <= 1e-12 * direct, (i, direct, gt_apd[i])

    csv_gt = gt_apd.copy()
    csv_gt[[3, 40, 77, 149]] = 0.0  # skipped by the storer (apde.py:18); singleton sets are 0 already
    apd_pred = (torch.from_numpy(gt_apd).float() * (1 + 0.2 * apd_noise) + 0.5).float()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mmapd_GT.csv")
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["id", "gt_APD"])
            for i, v in enumerate(csv_gt):
                w.writerow([i, repr(float(v))])
        storer = apde_mod.MetricStorerAPDE(mmapd_gt_path=path)
        for a in range(0, N, BATCH):
            storer.update(apd_pred[a:a + BATCH])
        apde = float(storer.compute())
    skipped = int((csv_gt == 0).sum())
    print(f"apde {apde:.9f} over {N - skipped} of {N} segments ({skipped} with gt_APD 0)")

    out = os.path.join(HERE, "mmgt.npz")
    np.savez_compressed(out, obs=obs.numpy(), thr=np.float64(THR), row_ptr=row_ptr, col=col, futures=futures.numpy(),
                        gt_apd=gt_apd, csv_gt_apd=csv_gt, apd_pred=apd_pred.numpy(), apde=np.float64(apde))
    print(f"wrote {out}: {os.path.getsize(out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
