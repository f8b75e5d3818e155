"""FID without a device: a float64 restatement of the reference's classifier (fid_classifier.py:38-53) and of
its statistics (fid.py:7-11) against tests/golden/fid.npz -- the reference's own float32 activations and fid()
values (gen_golden_fid.py) --, metrics.frechet_distance, the C ABI's host-side refusals, the checkpoint
loader and the accumulator's merge / all_reduce.

Tolerances.  Activations: 2e-5 absolute, the bar tests/test_gpu_kernels.py holds kernels to against float64
and about 30x the reference's own float32-vs-float64 difference on these cases (1.5e-7 .. 7.3e-7).
frechet_distance against the reference's scipy.linalg.sqrtm form: 1e-6 relative."""
import ctypes
import functools
import os
import re
import socket

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from skeletondiffusion_amd import _lib, checkpoint, metrics, synthetic
from skeletondiffusion_amd._lib import SkelDiffError

H, FEAT = 128, 30
# gen_golden_fid.py CASES: name -> ((B, S, T, J), fid() stored)
CASES = {"long": ((2, 3, 100, 16), False), "short": ((40, 2, 7, 16), True), "one": ((33, 2, 1, 16), True),
         "j15": ((5, 3, 4, 15), False)}
FID_SYMBOLS = ("sd_fid_workspace_bytes", "sd_fid_features", "sd_fid_stats_workspace_bytes", "sd_fid_stats_update")


@functools.lru_cache(maxsize=None)
def fid_state_dict(J=16):
    """gen_golden_fid.py:classifier restated: every parameter of ClassifierForFID(input_size=3 J), in sorted
    name order i = 0, 1, ..., is synthetic.uniform(shape, seed=100 + i, low=-0.15, high=0.15)."""
    shapes = {"linear1.weight": (FEAT, H), "linear1.bias": (FEAT,), "linear2.weight": (15, FEAT), "linear2.bias": (15,)}
    for l, k in ((0, 3 * J), (1, H)):
        shapes.update({f"recurrent.weight_ih_l{l}": (3 * H, k), f"recurrent.weight_hh_l{l}": (3 * H, H),
                       f"recurrent.bias_ih_l{l}": (3 * H,), f"recurrent.bias_hh_l{l}": (3 * H,)})
    return {n: torch.from_numpy(synthetic.uniform(shapes[n], seed=100 + i, low=-0.15, high=0.15))
            for i, n in enumerate(sorted(shapes))}


@functools.lru_cache(maxsize=None)
def fid_inputs(B, S, T, J):
    """gen_golden_fid.py:inputs restated: (pred, target, h0 of pred, h0 of the ground truth)."""
    return (0.4 * torch.from_numpy(synthetic.normal((B, S, T, J, 3), 11)), 0.4 * torch.from_numpy(synthetic.normal((B, T, J, 3), 12)),
            torch.from_numpy(synthetic.normal((2, B * S, H), 13)), torch.from_numpy(synthetic.normal((2, B, H), 14)))


def R_features(sd, x, h0=None):
    """float64 restatement of get_fid_features: x (rows, frames, input_size), h0 (2, rows, 128) or None (zeros)
    -> (rows, 30).  torch.nn.GRU's cell: gates r, z, n; biases on both sides; r inside the n gate's hidden term."""
    x = x.double()
    rows, frames, _ = x.shape
    h = [torch.zeros(rows, H, dtype=torch.float64) if h0 is None else h0[l].double() for l in range(2)]
    p = {k: v.double() for k, v in sd.items()}
    for t in range(frames):
        inp = x[:, t]
        for l in range(2):
            gi = inp @ p[f"recurrent.weight_ih_l{l}"].T + p[f"recurrent.bias_ih_l{l}"]
            gh = h[l] @ p[f"recurrent.weight_hh_l{l}"].T + p[f"recurrent.bias_hh_l{l}"]
            r = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h[l] = (1 - z) * n + z * h[l]
            inp = h[l]
    return torch.tanh(h[1] @ p["linear1.weight"].T + p["linear1.bias"])


def state_of(acts):
    """(count, sum x, sum x x^T) of (rows, feat) activations, float64 on the host."""
    a = torch.as_tensor(np.asarray(acts), dtype=torch.float64)
    return torch.cat([torch.tensor([float(a.shape[0])], dtype=torch.float64), a.sum(0), (a.T @ a).reshape(-1)])


@functools.lru_cache(maxsize=None)
def restated(name):
    """The float64 restatement's (pred, gt) activations of a fixture case, computed once."""
    (B, S, T, J), _ = CASES[name]
    pred, target, hp, hg = fid_inputs(B, S, T, J)
    sd = fid_state_dict(J)
    return (R_features(sd, pred.reshape(B * S, T, 3 * J), hp).numpy(), R_features(sd, target.reshape(B, T, 3 * J), hg).numpy())


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference_activations(name):
    z = golden("fid")
    rp, rg = restated(name)
    for tag, got, ref in (("pred", rp, z[f"{name}_pred_act"]), ("gt", rg, z[f"{name}_gt_act"])):
        err = float(np.abs(got - ref).max())
        print(f"{name} {tag}: max |restatement - reference| = {err:.2e}")
        assert ref.dtype == np.float32 and got.shape == ref.shape and err < 2e-5


@pytest.mark.parametrize("name", [n for n, (_, f) in CASES.items() if f])
def test_frechet_distance_matches_reference_fid(name):
    """fid(gt, pred) of fid.py:70-73 on the reference's activations: np.mean (float32), np.cov (float64)."""
    z = golden("fid")
    g, p = z[f"{name}_gt_act"], z[f"{name}_pred_act"]
    got = metrics.frechet_distance(np.mean(g, axis=0), np.cov(g, rowvar=False), np.mean(p, axis=0), np.cov(p, rowvar=False))
    ref = float(z[f"{name}_fid"])
    print(f"{name}: frechet_distance {got:.9f}, reference fid {ref:.9f}, relative {abs(got - ref) / ref:.2e}")
    assert isinstance(got, float) and abs(got - ref) <= 1e-6 * abs(ref)
    # the accumulator's statistics from (count, sum, sum of products) give the same value
    acc = metrics.FIDAccumulator(feat_size=FEAT, device="cpu")
    acc.state_pred += state_of(p)
    acc.state_gt += state_of(g)
    assert abs(acc.compute() - ref) <= 1e-6 * abs(ref)


def test_header_binding_and_library_agree_on_fid_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "skeldiff.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z_0-9]+)\s*\(", src))
    lib = _lib.lib()
    for name in FID_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.sd_abi_version() == 4  # additive, as sd_best_sample and sd_realism were
    fields = [n for n, _ in _lib.SDFidClassifierDesc._fields_]
    body = re.search(r"typedef struct sd_fid_classifier_desc \{(.*?)\}", src, flags=re.S).group(1)
    assert fields == re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", body)


def _desc(input_size=48, hidden_size=H, feat_size=FEAT):
    return _lib.SDFidClassifierDesc(input_size, hidden_size, feat_size, *([None] * 10))


@pytest.mark.parametrize("kw, frames, word", [
    (dict(hidden_size=64), 7, b"hidden_size"), (dict(hidden_size=256), 7, b"hidden_size"),
    (dict(feat_size=33), 7, b"feat_size"), (dict(feat_size=0), 7, b"feat_size"),
    (dict(input_size=0), 7, b"input_size"), (dict(input_size=65), 7, b"input_size"),
    (dict(), 0, b"frames"),
])
def test_invalid_shapes_are_refused_on_the_host(kw, frames, word):
    """Every device pointer is NULL: a refusal can only have happened before any device call."""
    lib = _lib.lib()
    d = _desc(**kw)
    rc = lib.sd_fid_features(ctypes.byref(d), None, 4, frames, None, None, None, 1 << 30, None)
    assert rc == -1 and word in lib.sd_last_error(), lib.sd_last_error()
    if word != b"frames":
        assert lib.sd_fid_workspace_bytes(ctypes.byref(d), 4) == 0 and word in lib.sd_last_error()


def test_short_workspace_and_empty_calls_on_the_host():
    lib = _lib.lib()
    d = _desc()
    need = lib.sd_fid_workspace_bytes(ctypes.byref(d), 4)
    assert need >= 4 * (3 * H * (48 + 3 * H) + FEAT * H + 8 * H + FEAT)  # at least the 166 k parameters
    assert lib.sd_fid_features(ctypes.byref(d), None, 4, 7, None, None, None, need - 1, None) == -1
    assert b"workspace_bytes" in lib.sd_last_error()
    assert lib.sd_fid_features(ctypes.byref(d), None, 4, 7, None, None, None, need, None) == -1
    assert b"null" in lib.sd_last_error()
    assert lib.sd_fid_features(ctypes.byref(d), None, -1, 7, None, None, None, need, None) == -1
    assert b"rows" in lib.sd_last_error()
    assert lib.sd_fid_features(ctypes.byref(d), None, 0, 7, None, None, None, 0, None) == 0  # rows == 0 launches nothing
    # statistics
    assert lib.sd_fid_stats_update(None, 4, 33, None, None, 1 << 20, None) == -1 and b"feat" in lib.sd_last_error()
    assert lib.sd_fid_stats_update(None, 4, 0, None, None, 1 << 20, None) == -1 and b"feat" in lib.sd_last_error()
    assert lib.sd_fid_stats_update(None, -1, FEAT, None, None, 1 << 20, None) == -1 and b"rows" in lib.sd_last_error()
    sneed = lib.sd_fid_stats_workspace_bytes(300, FEAT)
    assert sneed == 2 * (FEAT + FEAT * FEAT) * 8  # two chunks of 256 rows
    assert lib.sd_fid_stats_update(None, 300, FEAT, None, None, sneed - 1, None) == -1
    assert b"workspace_bytes" in lib.sd_last_error()
    assert lib.sd_fid_stats_update(None, 300, FEAT, None, None, sneed, None) == -1 and b"null" in lib.sd_last_error()
    assert lib.sd_fid_stats_update(None, 0, FEAT, None, None, 0, None) == 0


def test_load_fid_classifier_round_trip(tmp_path):
    sd = fid_state_dict(16)
    torch.save({"model": dict(sd)}, tmp_path / "h36m_classifier.pth")
    for where in (tmp_path, tmp_path / "h36m_classifier.pth"):
        c = checkpoint.load_fid_classifier(str(where), "cpu")
        assert isinstance(c, metrics.FIDClassifier)
        assert (c.input_size, c.hidden_size, c.feat_size) == (48, H, FEAT)
        for k in metrics._FID_KEYS:
            assert torch.equal(c._w[k], sd[k])
    with pytest.raises(KeyError, match="linear1.bias"):
        metrics.FIDClassifier({k: v for k, v in sd.items() if k != "linear1.bias"}, "cpu")


def test_cpu_classifier_and_cpu_tensor_raise():
    c = metrics.FIDClassifier(fid_state_dict(16), "cpu")
    with pytest.raises(SkelDiffError):
        c.features(torch.zeros(2, 3, 16, 3))
    with pytest.raises(SkelDiffError):
        c.get_fid_features(torch.zeros(2, 48, 3))


def _one_shot(z, name):
    g, p = z[f"{name}_gt_act"], z[f"{name}_pred_act"]
    return state_of(p), state_of(g), float(z[f"{name}_fid"])


def test_accumulator_merge_equals_one_shot():
    z = golden("fid")
    sp, sg, ref = _one_shot(z, "short")
    p, g = z["short_pred_act"], z["short_gt_act"]
    parts = []
    for lo, hi, glo, ghi in ((0, 7, 0, 3), (7, 50, 3, 29), (50, 80, 29, 40)):
        a = metrics.FIDAccumulator(feat_size=FEAT, device="cpu")
        a.state_pred += state_of(p[lo:hi])
        a.state_gt += state_of(g[glo:ghi])
        parts.append(a)
    total = metrics.FIDAccumulator(feat_size=FEAT, device="cpu")
    for a in parts:
        assert total.merge(a) is total
    scale = float(sp.abs().max())
    assert float((total.state_pred - sp).abs().max()) <= 1e-12 * scale and float((total.state_gt - sg).abs().max()) <= 1e-12 * scale
    assert abs(total.compute() - ref) <= 1e-6 * ref
    total.reset()
    assert float(total.state_pred.abs().max()) == 0 and float(total.state_gt.abs().max()) == 0


def test_fewer_than_two_rows_raises_by_name():
    z = golden("fid")
    acc = metrics.FIDAccumulator(feat_size=FEAT, device="cpu")
    with pytest.raises(ValueError, match="at least 2 rows"):
        acc.compute()
    acc.state_pred += state_of(z["short_pred_act"])
    acc.state_gt += state_of(z["short_gt_act"][:1])  # np.cov of one row is NaN in the reference
    with pytest.raises(ValueError, match="at least 2 rows"):
        acc.compute()


# ---- all_reduce over gloo, world size 2 (modelled on tests/test_distributed.py) --------------------------
def _reduce_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    z = golden("fid")
    p, g = z["short_pred_act"], z["short_gt_act"]
    acc = metrics.FIDAccumulator(feat_size=FEAT, device="cpu")
    acc.state_pred += state_of(p[:31] if rank == 0 else p[31:])  # uneven shards
    acc.state_gt += state_of(g[:17] if rank == 0 else g[17:])
    acc.all_reduce()
    q.put((rank, acc.state_pred.numpy(), acc.state_gt.numpy(), acc.compute()))
    dist.barrier()
    dist.destroy_process_group()


def test_accumulator_all_reduce_two_ranks_equals_one_shot():
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=300) for _ in range(2)]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    sp, sg, ref = _one_shot(golden("fid"), "short")
    scale = float(sp.abs().max())
    for _, gp, gg, value in got:
        assert np.abs(gp - sp.numpy()).max() <= 1e-12 * scale and np.abs(gg - sg.numpy()).max() <= 1e-12 * scale
        assert abs(value - ref) <= 1e-6 * ref
