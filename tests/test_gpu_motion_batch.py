"""On-device motion batches on the MI355X: sd_motion_batch / sd_motion_draws through
skeletondiffusion_amd.data.DeviceMotionData, against the reference's fixture (tests/golden/motion_batch.npz, its
recorded draws supplied) and against the torch-op restatement of tests/motion_batch_cases.py computed on the CPU.

Bounds (derived, not measured; M is the largest raw |coordinate| of the case, b the pose box, 1 without one):
  unrotated, noise-free samples   bitwise: every step is one correctly rounded f32 operation in both
  rotated samples                 32 * 2^-24 * M / b.  A rotated value is a two-term product sum with coefficients
                                  rounded to f32: in any evaluation order, FMA included, within 4 roundings of exact;
                                  doubled four times, for |x| + |y| <= 2 M, for the two implementations, for the two
                                  rotated values of the centring difference, for the subtraction and the division
  noisy observation samples       4 * 2^-24 * M / b: the supplied noise is the f32 rounding of the reference's float64
                                  product; one rounding each of the noise, the sum, the difference and the division
"""
import numpy as np
import pytest
import torch

import motion_batch_cases as C

pytestmark = pytest.mark.gpu

LENGTHS = (400, 333, 257)  # 954 segments at obs 5 + pred 7: 318 samples at stride 3
NOISY_TRAIN = dict(C.TRAIN, if_noisy_obs=True, noise_level=0.3, noise_std=0.03)
_cache = {}


def big_data(J, cuda):
    """The same 990 frames at joint count J with the release-style train settings and a noisy observation."""
    from skeletondiffusion_amd.data import DeviceMotionData

    if J not in _cache:
        _cache[J] = DeviceMotionData(C.synthetic_clips(LENGTHS, J, 7 + J), 5, 7, device=cuda, clip_class=[2, 0, 1], **NOISY_TRAIN)
    return _cache[J]


def big_batch(J, cuda):
    """(indices, batch of the first 300 samples at seed 11, epoch 3), computed once."""
    key = ("batch", J)
    if key not in _cache:
        idx = torch.arange(300, device=cuda)
        _cache[key] = (idx, big_data(J, cuda).batch(idx, train=True, seed=11, epoch=3))
    return _cache[key]


@pytest.mark.parametrize("case", list(C.CASES))
def test_against_the_reference_with_supplied_draws(case, cuda):
    data, a = C.case_data(case, cuda)
    train = C.CASES[case][1]
    obs, pred, extra = data.batch(a["sample_idx"].tolist(), train=train, draws=C.case_draws(a))
    assert obs.dtype == pred.dtype == torch.float32 and obs.is_cuda
    assert tuple(obs.shape) == a["obs"].shape and tuple(pred.shape) == a["pred"].shape
    for k in ("sample_idx", "segment_idx", "clip_idx", "init", "end"):
        assert extra[k].dtype == torch.int64 and extra[k].is_cuda, k
    seg = extra["segment_idx"].cpu().numpy()
    assert np.array_equal(seg, a["segment_idx"])
    assert np.array_equal(extra["sample_idx"].cpu().numpy(), a["sample_idx"])
    for col, k in enumerate(("clip_idx", "init", "end")):
        assert np.array_equal(extra[k].cpu().numpy(), a["segments"][a["segment_idx"], col]), k
    obs, pred = obs.cpu().numpy(), pred.cpu().numpy()
    b = data.pose_box_size if data.motion_repr_type == "SkeletonRescalePose" else 1.0
    M = C.raw_max(a)
    plain = a["degrees"] < 0
    err_rot = max(float(np.abs(obs - a["obs"])[~plain].max(initial=0)), float(np.abs(pred - a["pred"])[~plain].max(initial=0)))
    err_noisy = float(np.abs(obs - a["obs"]).max()) if data.if_noisy_obs else 0.0
    print(f"{case}: {int(plain.sum())} unrotated, {int((~plain).sum())} rotated; rotated max error {err_rot:.3e} "
          f"(bound {32 * 2.0 ** -24 * M / b:.3e}), noisy max error {err_noisy:.3e} (bound {4 * 2.0 ** -24 * M / b:.3e})")
    assert C.bits_equal(pred[plain], a["pred"][plain])
    if data.if_noisy_obs:
        clean = ~a["noise_mask"]
        assert C.bits_equal(obs[clean], a["obs"][clean])
        assert err_noisy <= 4 * 2.0 ** -24 * M / b
    else:
        assert C.bits_equal(obs[plain], a["obs"][plain])
    if train:
        assert int(plain.sum()) >= 8 and int(((a["degrees"] >= 0) & (a["degrees"] % 90 != 0)).sum()) >= 8
        assert err_rot <= 32 * 2.0 ** -24 * M / b
    # the kernel and the restatement round alike: the whole batch, rotated and noisy samples included
    r_obs, r_pred, r_seg = C.restate_data(data, a["sample_idx"], train=train, draws=C.case_draws(a))
    assert C.bits_equal(obs, r_obs) and C.bits_equal(pred, r_pred) and np.array_equal(seg, r_seg.numpy())


@pytest.mark.parametrize("J", [17, 52])
def test_philox_path_equals_supplied_path(J, cuda):
    data = big_data(J, cuda)
    idx, (obs, pred, extra) = big_batch(J, cuda)
    d = data.draws(idx, 11, 3)
    obs2, pred2, extra2 = data.batch(idx, train=True, draws=d)
    assert C.bits_equal(obs, obs2) and C.bits_equal(pred, pred2)
    assert torch.equal(extra["segment_idx"], extra2["segment_idx"])
    assert d["offset"].shape == (300,) and d["mirror"].shape == (300, 2) and d["degrees"].shape == (300,)
    assert d["noise_mask"].shape == (300, 5, J - 1) and d["noise"].shape == (300, 5, J - 1, 3)
    assert d["mirror"].dtype == torch.bool and d["noise_mask"].dtype == torch.bool and d["noise"].dtype == torch.float32
    deg, off = d["degrees"].cpu(), d["offset"].cpu()
    assert int(deg.min()) >= -1 and int(deg.max()) < 360 and int(off.abs().max()) <= data.augmentation
    assert len(set(off.tolist())) == 2 * data.augmentation + 1 and bool((deg < 0).any()) and bool((deg >= 0).any())
    assert bool(d["mirror"].any(0).all()) and not bool(d["mirror"].all())
    if J == 17:  # 24,000 pairs: sigma = sqrt(0.3 * 0.7 / 24000) = 0.0030, 6 sigma: 0.282 .. 0.318
        assert d["noise_mask"].numel() == 24000
        freq = float(d["noise_mask"].float().mean())
        print(f"mask frequency {freq:.4f}")
        assert 0.282 <= freq <= 0.318
    # the noise is noise_std times a unit normal: mean 0 and deviation noise_std within 6 sigma of their estimates
    n = d["noise"].double().flatten()
    assert abs(float(n.mean())) <= 6 * 0.03 / n.numel() ** 0.5 and abs(float(n.std()) / 0.03 - 1) <= 6 / (2 * n.numel()) ** 0.5
    # and the supplied path takes the draws it is given: the CPU restatement with the same draws, bitwise
    r_obs, r_pred, r_seg = C.restate_data(data, idx.cpu(), train=True, draws={k: v.cpu() for k, v in d.items()})
    assert C.bits_equal(obs, r_obs) and C.bits_equal(pred, r_pred) and torch.equal(extra["segment_idx"].cpu(), r_seg)


def test_partition_invariance_and_determinism(cuda):
    data = big_data(17, cuda)
    idx, (obs, pred, extra) = big_batch(17, cuda)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(300)).to(cuda)
    got_obs, got_pred, got_seg = torch.empty_like(obs), torch.empty_like(pred), torch.empty_like(extra["segment_idx"])
    a = 0
    for size in (1, 7, 292):
        part = perm[a:a + size]
        o, p, e = data.batch(part, train=True, seed=11, epoch=3)
        got_obs[part], got_pred[part], got_seg[part] = o, p, e["segment_idx"]
        a += size
    assert a == 300
    assert C.bits_equal(got_obs, obs) and C.bits_equal(got_pred, pred) and torch.equal(got_seg, extra["segment_idx"])
    again = data.batch(idx, train=True, seed=11, epoch=3)
    assert C.bits_equal(again[0], obs) and C.bits_equal(again[1], pred)
    d3, d4, ds = data.draws(idx, 11, 3), data.draws(idx, 11, 4), data.draws(idx, 12, 3)
    for other in (d4, ds):  # another epoch, another seed: other draws
        assert not torch.equal(d3["noise"], other["noise"]) and not torch.equal(d3["degrees"], other["degrees"])
        assert not torch.equal(d3["noise_mask"], other["noise_mask"])
    assert not C.bits_equal(data.batch(idx, train=True, seed=11, epoch=4)[0], obs)
    # eval mode: no mirroring or rotation, the offset and the noise stay
    e_obs, e_pred, e_extra = data.batch(idx, train=False, seed=11, epoch=3)
    r = C.restate_data(data, idx.cpu(), train=False, draws={k: v.cpu() for k, v in d3.items()})
    assert C.bits_equal(e_obs, r[0]) and C.bits_equal(e_pred, r[1]) and torch.equal(e_extra["segment_idx"], extra["segment_idx"])
    assert torch.equal(extra["class_idx"].cpu(), torch.tensor([2, 0, 1])[extra["clip_idx"].cpu()])


def test_resident_data_is_untouched(cuda):
    data = big_data(52, cuda)
    frames, table = data.frames.clone(), data.seg_first.clone()
    idx = torch.arange(len(data), device=cuda)
    for epoch in range(3):
        data.batch(idx, train=True, seed=5, epoch=epoch)
        data.batch(idx, train=False, seed=5, epoch=epoch)
    assert C.bits_equal(data.frames, frames) and torch.equal(data.seg_first, table)


# (J_full, obs, pred, B, representation): the frame tile is 32 up to J = 21, 13 at J = 52, 10 at J = 64
EDGES = {
    "one_sample": (17, 5, 7, 1, "SkeletonRescalePose"),
    "obs_length_1": (17, 1, 7, 9, "SkeletonRescalePose"),
    "pred_length_1": (22, 6, 1, 9, "SkeletonRescalePose"),
    "tile_larger_than_segment": (21, 2, 3, 9, "SkeletonRescalePose"),
    "segment_is_one_tile": (17, 20, 12, 5, "SkeletonRescalePose"),
    "segment_one_more_than_a_tile_j17": (17, 20, 13, 5, "SkeletonRescalePose"),
    "segment_one_more_than_a_tile_j52": (52, 9, 5, 5, "SkeletonCenterPose"),
    "tile_straddles_obs_and_pred_j64": (64, 6, 15, 5, "SkeletonRescalePose"),
    "two_joints": (2, 40, 33, 7, "SkeletonRescalePose"),
    "sixty_four_joints": (64, 11, 10, 7, "SkeletonVanilla"),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_shape_edges_against_the_restatement(edge, cuda):
    from skeletondiffusion_amd import _lib
    from skeletondiffusion_amd.data import DeviceMotionData

    J, obs_len, pred_len, B, kind = EDGES[edge]
    tile = _lib.lib().sd_motion_batch_frame_tile(J)
    if edge.startswith("segment_one_more"):
        assert obs_len + pred_len == tile + 1
    if edge in ("tile_larger_than_segment", "one_sample"):
        assert obs_len + pred_len < tile
    if edge == "segment_is_one_tile":
        assert obs_len + pred_len == tile
    seg_len = obs_len + pred_len
    data = DeviceMotionData(C.synthetic_clips((seg_len + 9, seg_len + 1, seg_len + 14), J, 31 + J), obs_len, pred_len, device=cuda,
                            motion_repr_type=kind, pose_box_size=1.25, stride=2, augmentation=3, da_mirroring=0.5,
                            da_rotations=0.7, if_noisy_obs=True, noise_level=0.4, noise_std=0.05)
    assert len(data) >= B
    idx = list(range(len(data)))[::-1][:B]  # the last samples: the clamp at the end of the list among them
    for train in (True, False):
        obs, pred, extra = data.batch(idx, train=train, seed=77, epoch=2)
        assert tuple(obs.shape) == (B, obs_len, J - 1, 3) and tuple(pred.shape) == (B, pred_len, J - 1, 3)
        d = {k: v.cpu() for k, v in data.draws(idx, 77, 2).items()}
        r_obs, r_pred, r_seg = C.restate_data(data, idx, train=train, draws=d)
        assert torch.equal(extra["segment_idx"].cpu(), r_seg)
        assert C.bits_equal(obs, r_obs) and C.bits_equal(pred, r_pred)


def test_empty_batch_and_device_indices(cuda):
    data = big_data(17, cuda)
    obs, pred, extra = data.batch([], train=True, seed=1)
    assert tuple(obs.shape) == (0, 5, 16, 3) and tuple(pred.shape) == (0, 7, 16, 3) and extra["segment_idx"].numel() == 0
    with pytest.raises(IndexError):
        data.batch([len(data)], train=True)
    with pytest.raises(IndexError):
        data.batch(torch.tensor([-1]), train=True)
    # a device index out of range is the caller's error; the kernel still reads inside the table
    far = torch.tensor([-7, 10 ** 12], device=cuda)
    _, _, extra = data.batch(far, train=False, seed=1)
    assert extra["segment_idx"].tolist() == [0, data.nseg - 1]


def test_derived_tensors(cuda):
    from skeletondiffusion_amd import multimodal_gt
    from skeletondiffusion_amd.data import DeviceMotionData

    a = C.case_arrays("train_j17")
    plain = DeviceMotionData(C.case_clips(a), 5, 7, device=cuda)  # stride 1, no augmentation, no noise
    obs, pred, extra = plain.batch(torch.arange(plain.nseg, device=cuda), train=False)
    assert torch.equal(extra["segment_idx"].cpu(), torch.arange(plain.nseg))
    fut, last = plain.all_futures(), plain.last_obs()
    assert C.bits_equal(fut, pred) and C.bits_equal(last, obs[:, -1]) and last.is_contiguous()
    # a dataset with augmentation and noise gives the same unaugmented tensors
    data, _ = C.case_data("train_j17", cuda, if_noisy_obs=True)
    assert C.bits_equal(data.all_futures(), fut) and C.bits_equal(data.last_obs(), last)
    metric = data.representation.transform_to_metric_space(last)
    gt = multimodal_gt.get_multimodal_gt(metric, 0.5)
    assert len(gt) == plain.nseg
    sets = gt.to_dict()
    assert all(i in sets[i] for i in range(plain.nseg))
    apd = gt.gt_apd(fut)
    assert tuple(apd.shape) == (plain.nseg,) and bool(torch.isfinite(apd).all())


def test_batches_visit_every_sample_once(cuda):
    data = big_data(17, cuda)
    n = len(data)

    def epoch(**kw):
        return [(o, p, e) for o, p, e in data.batches(64, train=True, **kw)]

    run = epoch(shuffle=True, seed=4, epoch=1)
    assert [b[0].shape[0] for b in run] == [64] * (n // 64) + [n % 64]
    order = torch.cat([e["sample_idx"] for _, _, e in run]).cpu()
    assert sorted(order.tolist()) == list(range(n)) and order.tolist() != list(range(n))
    again = epoch(shuffle=True, seed=4, epoch=1)
    assert torch.equal(torch.cat([e["sample_idx"] for _, _, e in again]).cpu(), order)
    assert all(C.bits_equal(x[0], y[0]) and C.bits_equal(x[1], y[1]) for x, y in zip(run, again))
    other = torch.cat([e["sample_idx"] for _, _, e in epoch(shuffle=True, seed=4, epoch=2)]).cpu()
    assert sorted(other.tolist()) == list(range(n)) and not torch.equal(other, order)
    plain = epoch(shuffle=False, seed=4, epoch=1, drop_last=True)
    assert len(plain) == n // 64 and torch.cat([e["sample_idx"] for _, _, e in plain]).cpu().tolist() == list(range(n // 64 * 64))
    # a sample's data does not depend on where the permutation put it
    o, p, _ = data.batch(order.to(cuda), train=True, seed=4, epoch=1)
    assert C.bits_equal(torch.cat([b[0] for b in run]), o) and C.bits_equal(torch.cat([b[1] for b in run]), p)
