"""The multimodal ground truth without a device (multimodal_gt.MultimodalGT's dict and file halves,
metrics.APDEAccumulator, the C ABI's host-side refusals) against tests/golden/mmgt.npz: the reference's own
get_multimodal_gt adjacency, float64 apd table and MetricStorerAPDE value (gen_golden_mmgt.py).

Tolerance.  APDE: 1e-12 relative; both sides add at most 150 float64 terms of similar size."""
import ast
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import golden
from skeletondiffusion_amd import _lib, evaluation, metrics, multimodal_gt
from skeletondiffusion_amd._lib import SkelDiffError

MMGT_SYMBOLS = ("sd_cdist", "sd_set_mean_distance")
BATCHES = ((0, 64), (64, 128), (128, 150))  # gen_golden_mmgt.py: the storer's three updates


def reference_dict(z):
    rp, col = z["row_ptr"].tolist(), z["col"].tolist()
    return {i: set(col[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)}


def fixture_csr(device="cpu"):
    z = golden("mmgt")
    return multimodal_gt.MultimodalGT(torch.from_numpy(z["row_ptr"]), torch.from_numpy(z["col"]), device)


def test_symbols_are_bound():
    assert set(MMGT_SYMBOLS) <= set(_lib.EXPORTED)
    lib = _lib.lib()
    for name in MMGT_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7, name


def test_fixture_is_what_the_generator_describes():
    z = golden("mmgt")
    d = reference_dict(z)
    sizes = [len(v) for v in d.values()]
    assert len(d) == 150 and sum(sizes) == 1416 and min(sizes) == 1 and max(sizes) == 15
    assert all(i in d[i] for i in d) and all(i in d[j] for i in d for j in d[i])  # itself included, symmetric


def test_save_writes_the_reference_file(tmp_path):
    z = golden("mmgt")
    g = fixture_csr()
    assert g.to_dict() == reference_dict(z) and list(g.to_dict()) == list(range(150))
    path = tmp_path / "mmgt_test.txt"
    g.save(path)
    with open(path) as f:  # create_dataset_utils.py:46-49
        loaded = ast.literal_eval(json.load(f))
    assert loaded == reference_dict(z)


def test_load_reads_a_reference_file(tmp_path):
    z = golden("mmgt")
    path = tmp_path / "mmgt_test.txt"
    with open(path, "w") as f:  # create_dataset_utils.py:64-65
        json.dump(str(reference_dict(z)), f)
    g = multimodal_gt.MultimodalGT.load(path)
    assert torch.equal(g.row_ptr, torch.from_numpy(z["row_ptr"])) and torch.equal(g.col, torch.from_numpy(z["col"]))
    assert torch.equal(g.row_ptr_host, g.row_ptr) and len(g) == 150


def test_csr_is_validated():
    with pytest.raises(ValueError, match="row_ptr"):
        multimodal_gt.MultimodalGT([0, 2, 1], [0])
    with pytest.raises(ValueError, match="row_ptr"):
        multimodal_gt.MultimodalGT([0, 1, 3], [0, 1])


def test_mm_gt_lists_the_members_futures():
    z = golden("mmgt")
    g = fixture_csr()
    futures = torch.from_numpy(z["futures"])
    d = reference_dict(z)
    idx = [0, 5, 149]
    for i, got in zip(idx, g.mm_gt(futures, idx)):
        assert torch.equal(got, futures[sorted(d[i])])  # base_dataset.py:181-186, members ascending


def test_gt_apd_refuses_a_matrix_above_the_limit():
    z = golden("mmgt")
    with pytest.raises(SkelDiffError, match=r"N = 150.*limit of 1000 bytes"):
        fixture_csr().gt_apd(torch.from_numpy(z["futures"]), max_bytes=1000)


def _write_csv(path, ids, values):
    with open(path, "w") as f:
        f.write("id,gt_APD\n")
        for i, v in zip(ids, values):
            f.write(f"{i},{v!r}\n")


def test_from_csv_zero_to_nan_and_index_order(tmp_path):
    path = tmp_path / "mmapd_GT.csv"
    _write_csv(path, [2, 0, 1, 3], [5.0, 0.0, 7.5, 0])
    acc = metrics.APDEAccumulator.from_csv(path)
    g = acc.gt_apd
    assert g.dtype == torch.float64 and g[0] == 5.0 and g[2] == 7.5 and bool(torch.isnan(g[1])) and bool(torch.isnan(g[3]))
    acc.update(torch.tensor([6.0, 1.0]))  # sequential: file order (apde.py:34), the zero entry skipped
    assert acc.compute() == 1.0 and acc.index == 2
    acc.reset()
    acc.update(torch.tensor([6.0, 1.0, 9.0]), segment_idx=[1, 0, 2])  # by id: 7.5, nan, 5.0
    assert acc.compute() == (1.5 + 4.0) / 2


def _fed(acc, z, by_index=False, batches=BATCHES):
    pred = torch.from_numpy(z["apd_pred"])
    for a, b in batches:
        acc.update(pred[a:b], segment_idx=list(range(a, b)) if by_index else None)
    return acc


def test_apde_accumulator_matches_the_reference_storer(tmp_path):
    z = golden("mmgt")
    want = float(z["apde"])
    got = _fed(metrics.APDEAccumulator(torch.from_numpy(z["csv_gt_apd"])), z).compute()
    assert abs(got - want) <= 1e-12 * want, (got, want)
    assert _fed(metrics.APDEAccumulator(torch.from_numpy(z["csv_gt_apd"])), z, by_index=True).compute() == got
    path = tmp_path / "mmapd_GT.csv"
    _write_csv(path, range(150), z["csv_gt_apd"].tolist())
    factory, transform = evaluation.get_apde_storer(annotations_folder=str(tmp_path), device="cpu")
    assert _fed(factory(output_transform=transform), z).compute() == got
    first, second = (_fed(metrics.APDEAccumulator(torch.from_numpy(z["csv_gt_apd"])), z, True, part)
                     for part in (BATCHES[:1], BATCHES[1:]))
    merged = first.merge(second)
    assert abs(merged.compute() - got) <= 1e-12 * got and int(merged.count) == 145
    assert np.isnan(metrics.APDEAccumulator(torch.zeros(3)).compute())
    with pytest.raises(ValueError, match="table of 3"):
        metrics.APDEAccumulator(torch.ones(3)).update(torch.ones(4))


def test_cdist_rejects_bad_arguments_on_the_host():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for args, word in (((p, -1, p, 2, 3, p), b"m must"), ((p, 2, p, -1, 3, p), b"n must"), ((p, 2, p, 2, 0, p), b"features"),
                       ((None, 2, p, 2, 3, p), b"x1"), ((p, 2, None, 2, 3, p), b"x2"), ((p, 2, p, 2, 3, None), b"dist")):
        assert lib.sd_cdist(*args, None) == -1, args
        msg = lib.sd_last_error()
        assert msg.startswith(b"cdist:") and word in msg, msg
    # an empty shape launches nothing and needs no buffers
    assert lib.sd_cdist(None, 0, None, 5, 3, None, None) == 0 and lib.sd_cdist(None, 5, None, 0, 3, None, None) == 0


def test_set_mean_distance_rejects_bad_arguments_on_the_host():
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for args, word in (((p, -1, p, p, 2, p), b"n must"), ((p, 4, p, p, -1, p), b"nsets"), ((None, 4, p, p, 2, p), b"dist"),
                       ((p, 4, None, p, 2, p), b"row_ptr"), ((p, 4, p, None, 2, p), b"col"), ((p, 4, p, p, 2, None), b"out")):
        assert lib.sd_set_mean_distance(*args, None) == -1, args
        msg = lib.sd_last_error()
        assert msg.startswith(b"set_mean_distance:") and word in msg, msg
    assert lib.sd_set_mean_distance(None, 4, None, None, 0, None, None) == 0


def test_device_entry_points_refuse_host_tensors():
    x = torch.zeros(3, 4)
    with pytest.raises(SkelDiffError, match="ROCm tensor"):
        multimodal_gt.cdist(x, x)
    with pytest.raises(SkelDiffError, match="ROCm tensor"):
        multimodal_gt.get_multimodal_gt(torch.zeros(3, 16, 3), 0.5)
