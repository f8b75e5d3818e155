"""Host side of the on-device motion batches: the segment table and its clamp against the
reference's fixture, the C ABI and its argument checks, the refusals, MotionRepresentation on CPU tensors, and a
stand-alone emulation of the kernels' address arithmetic under AddressSanitizer.  No GPU; the device tests are in
tests/test_gpu_motion_batch.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import motion_batch_cases as C
from conftest import REPO
from skeletondiffusion_amd import _lib
from skeletondiffusion_amd._lib import SkelDiffError


@pytest.mark.parametrize("case", list(C.CASES))
def test_segment_table_len_and_clamp_equal_the_fixture(case):
    from skeletondiffusion_amd import data as D

    data, a = C.case_data(case, "cpu")
    assert data.nseg == len(a["segments"]) and len(data) == len(a["sample_idx"]) == data.nseg // data.stride
    assert np.array_equal(data.segments, a["segments"][:, :2])
    assert np.array_equal(data.segments[:, 1] + data.seg_length - 1, a["segments"][:, 2])
    first = np.concatenate([[0], np.cumsum(a["clip_lengths"])])[a["segments"][:, 0]] + a["segments"][:, 1]
    assert np.array_equal(data.seg_first.numpy(), first) and data.seg_first.dtype == torch.int64
    assert tuple(data.frames.shape) == a["clips"].shape and data.frames.dtype == torch.float32
    seg = D.segment_index(a["sample_idx"], a["offset"], data.stride, data.augmentation, data.nseg)
    assert np.array_equal(seg, a["segment_idx"])
    if case in C.TRAIN_CASES:
        assert seg[0] == 0 and seg[-1] == data.nseg - 1  # both ends of the list are reached
        assert data.stride * a["sample_idx"][-1] + data.augmentation + a["offset"][-1] > data.nseg - 1  # and clamped
    if case != "segments_j17":  # the generated list leaves out the last possible start of every clip
        lengths = a["clip_lengths"]
        assert data.nseg == int((lengths - data.seg_length).sum())
        assert not any((c, lengths[c] - data.seg_length) in set(map(tuple, data.segments.tolist())) for c in range(len(lengths)))


def test_explicit_segments_force_stride_and_augmentation():
    data, a = C.case_data("segments_j17", "cpu", stride=3, augmentation=2)
    assert (data.stride, data.augmentation) == (1, 0) and len(data) == len(a["segments"])
    clips = C.case_clips(a)
    from skeletondiffusion_amd.data import DeviceMotionData
    with pytest.raises(ValueError, match=r"segments\[1\]"):
        DeviceMotionData(clips, 5, 7, segments=[(0, 0), (1, 22)], device="cpu")  # 22 + 12 > 33


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "skeldiff.h")).read()
    assert re.search(r"\bint sd_motion_batch\(const float\* frames, int64_t total_frames", hdr)
    assert re.search(r"\bint sd_motion_draws\(const int64_t\* sample_idx, int64_t B", hdr)
    assert re.search(r"\bint32_t sd_motion_batch_frame_tile\(int32_t joints\)", hdr)
    for name in ("sd_motion_batch", "sd_motion_draws", "sd_motion_batch_frame_tile"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name), name
    assert re.search(r"#define SD_ABI_VERSION 4\b", hdr) and _lib.lib().sd_abi_version() == _lib.SD_ABI_VERSION == 4
    for name in ("SD_MOTION_VANILLA", "SD_MOTION_CENTER_POSE", "SD_MOTION_RESCALE_POSE"):
        assert re.search(rf"#define {name} {getattr(_lib, name)}\b", hdr)
    assert "motion_dataset.py" in hdr and "base_dataset.py" in hdr  # the reference lines it replaces are cited


def test_host_argument_checks():
    """sd_motion_batch / sd_motion_draws validate on the host, before any device call, and name the argument."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)  # a non-null address; the checks return before any use
    p = ctypes.addressof(buf)

    def batch(frames=p, total_frames=100, seg_first=p, nseg=10, sample_idx=p, B=4, joints=17, obs_len=5, pred_len=7, stride=1,
              augmentation=0, train=1, representation=2, pose_box_size=1.5, da_mirroring=0.5, da_rotations=0.5, noisy=0,
              noise_level=0.3, noise_std=0.03, rot_table=p, draws=(None,) * 5, obs=p, pred=p, segment_idx=p):
        return L.sd_motion_batch(frames, total_frames, seg_first, nseg, sample_idx, B, joints, obs_len, pred_len, stride,
                                 augmentation, train, representation, pose_box_size, da_mirroring, da_rotations, noisy,
                                 noise_level, noise_std, rot_table, 1, 0, *draws, obs, pred, segment_idx, None)

    def draws(sample_idx=p, B=4, joints=17, obs_len=5, augmentation=0, da_mirroring=0.5, da_rotations=0.5, noise_level=0.3,
              noise_std=0.03, offset=p, mirror=p, degrees=p, noise_mask=p, noise=p):
        return L.sd_motion_draws(sample_idx, B, joints, obs_len, augmentation, da_mirroring, da_rotations, noise_level,
                                 noise_std, 1, 0, offset, mirror, degrees, noise_mask, noise, None)

    nan = float("nan")
    both = ((dict(joints=1), b"joints"), (dict(joints=65), b"joints"), (dict(obs_len=0), b"obs_len"),
            (dict(augmentation=-1), b"augmentation"), (dict(da_mirroring=1.5), b"da_mirroring"),
            (dict(da_mirroring=-0.1), b"da_mirroring"), (dict(da_rotations=2.0), b"da_rotations"), (dict(da_rotations=nan), b"da_rotations"),
            (dict(noise_level=-1.0), b"noise_level"), (dict(noise_std=-1.0), b"noise_std"), (dict(sample_idx=None), b"sample_idx"),
            (dict(B=-1), b"B must"))
    only_batch = ((dict(pred_len=0), b"pred_len"), (dict(nseg=0), b"nseg"), (dict(pose_box_size=0.0), b"pose_box_size"),
                  (dict(pose_box_size=-1.5), b"pose_box_size"), (dict(pose_box_size=nan), b"pose_box_size"),
                  (dict(representation=3), b"representation"), (dict(representation=-1), b"representation"),
                  (dict(stride=0), b"stride"), (dict(total_frames=11), b"total_frames"),
                  (dict(frames=None), b"frames"), (dict(seg_first=None), b"seg_first"), (dict(rot_table=None), b"rot_table"),
                  (dict(obs=None), b"obs is null"), (dict(pred=None), b"pred is null"), (dict(segment_idx=None), b"segment_idx"),
                  (dict(draws=(None, p, p, None, None)), b"draw_offset"), (dict(draws=(p, None, p, None, None)), b"draw_mirror"),
                  (dict(draws=(p, p, None, None, None)), b"draw_degrees"),
                  (dict(draws=(p, p, p, None, p), noisy=1), b"draw_noise_mask"), (dict(draws=(p, p, p, p, None), noisy=1), b"draw_noise is"))
    only_draws = ((dict(offset=None), b"offset"), (dict(mirror=None), b"mirror"), (dict(degrees=None), b"degrees"),
                  (dict(noise=None), b"noise_mask and noise"), (dict(noise_mask=None), b"noise_mask and noise"))
    for call, cases in ((batch, both + only_batch), (draws, both + only_draws)):
        for kw, word in cases:
            assert call(**kw) == -1, kw
            assert word in L.sd_last_error(), (kw, L.sd_last_error())
    # B = 0: nothing launched, whatever the pointers
    assert batch(B=0, frames=None, seg_first=None, sample_idx=None, obs=None, pred=None, segment_idx=None) == 0
    assert draws(B=0, sample_idx=None, offset=None, mirror=None, degrees=None, noise_mask=None, noise=None) == 0
    for joints, tile in ((2, 32), (17, 32), (21, 32), (22, 31), (52, 13), (64, 10)):
        assert L.sd_motion_batch_frame_tile(joints) == tile
    assert L.sd_motion_batch_frame_tile(1) == -1 and L.sd_motion_batch_frame_tile(65) == -1


def test_refusals_carry_their_name():
    from skeletondiffusion_amd.data import DeviceMotionData, MotionRepresentation

    clips = [np.zeros((20, 17, 3), np.float32)]
    with pytest.raises(SkelDiffError, match="SkeletonDiscreteCosineTransform"):
        DeviceMotionData(clips, 5, 7, motion_repr_type="SkeletonDiscreteCosineTransform", device="cpu")
    with pytest.raises(SkelDiffError, match="SkeletonDiscreteCosineTransform"):
        MotionRepresentation("SkeletonDiscreteCosineTransform", 17)
    with pytest.raises(SkelDiffError, match="if_consider_hip"):
        DeviceMotionData(clips, 5, 7, if_consider_hip=True, device="cpu")
    with pytest.raises(SkelDiffError, match="if_consider_hip"):
        MotionRepresentation("SkeletonRescalePose", 17, if_consider_hip=True)
    with pytest.raises(SkelDiffError, match="normalize_data"):
        DeviceMotionData(clips, 5, 7, normalize_data=True, device="cpu")
    with pytest.raises(SkelDiffError, match="float64"):
        DeviceMotionData([np.zeros((20, 17, 3), np.float64)], 5, 7, device="cpu")
    with pytest.raises(TypeError, match="use_vel"):
        DeviceMotionData(clips, 5, 7, use_vel=True, device="cpu")
    data = DeviceMotionData(clips, 5, 7, device="cpu")  # a module on the CPU: its tables exist, its engine does not
    assert len(data) == 8
    for call in (lambda: data.batch([0], train=False), lambda: data.draws([0], 1, 0), data.all_futures, data.last_obs,
                 lambda: next(data.batches(4, train=True, shuffle=True, seed=1, epoch=0))):
        with pytest.raises(SkelDiffError, match="HIP engine"):
            call()


def test_kernel_addresses_in_bounds_under_asan(tmp_path):
    """tests/host/motion_batch_emulation.cpp walks every workgroup x thread x load / store of the two kernels with
    the kernels' own address functions (csrc/sd_motion_batch_addr.h): on real heap buffers at the fixture's shapes
    and the shape edges under AddressSanitizer + UBSan, arithmetically at 1,024 x (25 + 100) x 17 and
    512 x (30 + 120) x 52."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "motion_batch_emulation")
    src = os.path.join(REPO, "tests", "host", "motion_batch_emulation.cpp")
    # the sanitizer runtime is linked statically (g++ -static-libasan; clang's default), so the program
    # needs nothing preloaded and does not mind what its environment preloads
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or "c++" == os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "motion batch emulation ok" in r.stdout


def _whole_segments(a):
    """(B, seg, J, 3): the raw frames of every sample's segment."""
    first = np.concatenate([[0], np.cumsum(a["clip_lengths"])])[a["segments"][:, 0]] + a["segments"][:, 1]
    seg_len = int(a["obs"].shape[1] + a["pred"].shape[1])
    return torch.from_numpy(a["clips"])[torch.from_numpy(first[a["segment_idx"]])[:, None] + torch.arange(seg_len)[None]]


@pytest.mark.parametrize("case", list(C.CASES))
def test_motion_representation_equals_the_fixture_bitwise(case):
    """Unrotated, noise-free data through MotionRepresentation on CPU tensors gives the reference's bits (the
    mirroring is a sign, exact); the observation's noise-free pairs too in the noisy case."""
    from skeletondiffusion_amd.data import MotionRepresentation

    data, a = C.case_data(case, "cpu")
    rep = MotionRepresentation(data.motion_repr_type, data.num_joints, data.pose_box_size)
    x = _whole_segments(a)
    sign = torch.where(torch.from_numpy(a["mirror"]), -1.0, 1.0)
    x = torch.cat([x[..., :2] * sign[:, None, None, :], x[..., 2:]], -1)
    got = rep.tranform_to_input_space(x)
    assert got.shape[-2] == data.num_joints - 1
    want = torch.from_numpy(np.concatenate([a["obs"], a["pred"]], 1))
    plain = torch.from_numpy(a["degrees"] < 0)
    assert int(plain.sum()) >= 8
    clean = torch.ones(want.shape[:3], dtype=torch.bool)
    clean[:, :data.obs_length] = ~torch.from_numpy(a["noise_mask"])
    keep = (plain[:, None, None] & clean)[..., None].expand_as(want)
    assert C.bits_equal(got[keep], want[keep])
    assert rep.if_add_zero_pad_center_hip(got).shape[-2] == data.num_joints
    assert bool((rep.if_add_zero_pad_center_hip(got)[..., 0, :] == 0).all())
    assert rep.if_add_zero_pad_center_hip(x) is x


@pytest.mark.parametrize("case", list(C.CASES))
def test_restatement_against_the_reference(case):
    """tests/motion_batch_cases.py:restate, the yardstick of the GPU shape-edge tests, against the reference with
    the recorded draws, under the bounds the GPU test holds the kernel to."""
    data, a = C.case_data(case, "cpu")
    obs, pred, seg = C.restate_data(data, a["sample_idx"], train=C.CASES[case][1], draws=C.case_draws(a))
    assert np.array_equal(seg.numpy(), a["segment_idx"])
    scale = data.pose_box_size if data.motion_repr_type == "SkeletonRescalePose" else 1.0
    M = C.raw_max(a)
    plain = a["degrees"] < 0
    assert C.bits_equal(pred[plain], a["pred"][plain])
    err_rot = max(float(np.abs(obs.numpy() - a["obs"])[~plain].max(initial=0)), float(np.abs(pred.numpy() - a["pred"])[~plain].max(initial=0)))
    assert err_rot <= 32 * 2.0 ** -24 * M / scale
    if data.if_noisy_obs:
        assert float(np.abs(obs.numpy() - a["obs"]).max()) <= 4 * 2.0 ** -24 * M / scale
        clean = ~a["noise_mask"]
        assert C.bits_equal(obs[torch.from_numpy(clean)], a["obs"][clean])
    else:
        assert C.bits_equal(obs[plain], a["obs"][plain])


@pytest.mark.parametrize("kind", ["SkeletonCenterPose", "SkeletonRescalePose", "SkeletonVanilla"])
def test_metric_space_round_trip(kind):
    """transform_to_metric_space(tranform_to_input_space(x)) is the hip-centred input: bitwise for SkeletonCenterPose;
    for SkeletonRescalePose within one rounding step of the multiplication: r = fl(q b) is the centred value c or
    one of its two float32 neighbours.  (c is a float32; q = fl(c / b) is within half an ulp of c / b, so q b is
    within b / 2 = 0.75 ulp(q) <= 0.75 ulp(c) of c, and rounding the product adds at most half an ulp: r, a
    float32 within 1.25 ulp of the float32 c, is at most one step from it.)"""
    from skeletondiffusion_amd.data import MotionRepresentation

    a = C.case_arrays("train_j22")
    x = torch.from_numpy(a["clips"])
    rep = MotionRepresentation(kind, 22, 1.5)
    back = rep.transform_to_metric_space(rep.tranform_to_input_space(x))
    if kind == "SkeletonVanilla":
        assert C.bits_equal(back, x[..., 1:, :])
        return
    centred = (x - x[..., 0:1, :])[..., 1:, :]
    if kind == "SkeletonCenterPose":
        assert C.bits_equal(back, centred)
    else:
        inf = torch.full_like(centred, float("inf"))
        near = (back == centred) | (back == torch.nextafter(centred, inf)) | (back == torch.nextafter(centred, -inf))
        print("round trip: values one float32 step off:", int((back != centred).sum()), "of", back.numel())
        assert bool(near.all())
