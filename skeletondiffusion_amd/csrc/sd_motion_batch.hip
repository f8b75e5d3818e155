// Motion batches on the device: what the reference's data path does per item on the
// host, for a whole batch in one pass over clips that stay resident in device memory:
//   segment lookup with the augmentation offset and its clamp     base_dataset.py:109-116, :164-177
//   observation noise (add_noise)                                  motion_dataset.py:11-19, :187-188
//   mirroring and the rotation about z (data_augmentation)         motion_dataset.py:129-165
//   centring on the hip, the pose box, dropping the root           skeleton/motion/{utils,centerpose,rescalepose,base}.py
//   default_collate and the host-to-device copy                    (none: the batch is written where it is used)
// Two kernels:
//   k_motion_batch   one workgroup per (sample, tile of frames).  Thread 0 reads or draws the sample's
//                    decisions (they are workgroup-uniform) and looks the segment up; the tile's raw
//                    frames, one contiguous span, go to LDS with 16-byte loads from the span's first
//                    16-byte boundary on; one thread per (frame, joint >= 1) transforms from LDS, where
//                    the frame's hip is at hand, into a second LDS buffer in output order; the obs part
//                    and the pred part of the tile are then written as contiguous spans, with 16-byte
//                    stores from each span's first 16-byte boundary on.
//   k_motion_draws   the same decisions as tensors (one workgroup per sample).
// Every offset, LDS index and loop bound comes from sd_motion_batch_addr.h, which also holds the
// Philox quad map; tests/host/motion_batch_emulation.cpp walks the same functions.
//
// Arithmetic.  f32, one operation at a time, so the supplied-draw path, the Philox path and a plain
// f32 restatement round alike: x + noise; -x; c x - s y and s x + c y as two products and a difference
// / sum; x - hip; a correctly rounded division by pose_box_size.  Contraction is switched off by the
// pragma below, which covers the operators written in this file only: the __fmul_rn / __fadd_rn
// helpers of the HIP headers are defined ahead of it, keep their contract flag when inlined and were
// fused into v_fma_f32 here, so the arithmetic is written with plain operators.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_motion_batch_addr.h"
#include "sd_philox.h"

namespace sd {

namespace {

using namespace motion;

struct MotionArgs {
    const float* frames; int64_t total_frames;
    const int64_t* seg_first; int64_t nseg;
    const int64_t* sample_idx;
    int J, obs_len, pred_len;
    int64_t stride, augmentation;
    int train, repr;
    float box, p_mirror, p_rot;
    int noisy; float noise_level, noise_std;
    const float* rot;  // cos of 0..359 degrees, then sin of 0..359 degrees
    uint64_t seed; int epoch;
    // supplied draws (all null: the Philox stream)
    int supplied;
    const int32_t* d_offset; const uint8_t* d_mirror; const int32_t* d_degrees;
    const uint8_t* d_mask; const float* d_noise;
    float* obs; float* pred; int64_t* segment_idx;
};

struct SampleDraw {
    int offset, mirror0, mirror1, degrees;  // degrees -1: no rotation
};

__device__ __forceinline__ SampleDraw draw_sample(uint64_t seed, uint64_t row, int epoch, int64_t A, float p_mirror,
                                                  float p_rot) {
    const uint4 q = philox_at(seed, row, epoch, kQuadSample);
    SampleDraw d;
    d.offset = A ? (int)(q.x % (uint32_t)(2 * A + 1)) - (int)A : 0;
    d.mirror0 = u01(q.y) < p_mirror;
    d.mirror1 = u01(q.z) < p_mirror;
    d.degrees = u01(q.w) < p_rot ? (int)(philox_at(seed, row, epoch, kQuadDegrees).x % 360u) : -1;
    return d;
}

// noise_std * normal of the three coordinates of (frame t, joint j); true when the pair is hit
__device__ __forceinline__ bool draw_noise(uint64_t seed, uint64_t row, int epoch, int J, int t, int j, float level,
                                           float std_, float& nx, float& ny, float& nz) {
    const uint4 q = philox_at(seed, row, epoch, noise_quad(J, t, j));
    const floatx2 a = box_muller(q.x, q.y), b = box_muller(q.z, q.w);
    nx = std_ * a.x;
    ny = std_ * a.y;
    nz = std_ * b.x;
    const uint32_t m = (q.x & 255u) | ((q.y & 255u) << 8) | ((q.z & 255u) << 16) | ((q.w & 255u) << 24);
    return u01(m) < level;
}

__device__ __forceinline__ void load_span(const float* __restrict__ src, int N, float* __restrict__ dst, int tid) {
    int head, quads;
    span_split((uint64_t)(uintptr_t)src, N, head, quads);
    for (int e = tid; e < head; e += kThreads) dst[e] = src[e];
    const floatx4* sq = reinterpret_cast<const floatx4*>(src + head);
    for (int q = tid; q < quads; q += kThreads) {
        const floatx4 v = sq[q];
        float* d = dst + head + 4 * q;  // the LDS side is 4-byte aligned only
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst[e] = src[e];
}

__device__ __forceinline__ void store_span(float* __restrict__ dst, const float* __restrict__ src, int N, int tid) {
    int head, quads;
    span_split((uint64_t)(uintptr_t)dst, N, head, quads);
    for (int e = tid; e < head; e += kThreads) dst[e] = src[e];
    floatx4* dq = reinterpret_cast<floatx4*>(dst + head);
    for (int q = tid; q < quads; q += kThreads) {
        const float* s = src + head + 4 * q;
        dq[q] = floatx4{s[0], s[1], s[2], s[3]};
    }
    for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst[e] = src[e];
}

__global__ __launch_bounds__(kThreads) void k_motion_batch(MotionArgs a) {
    __shared__ float raw[kStageFloats];
    __shared__ float outb[kStageFloats];
    __shared__ int64_t s_first;
    __shared__ int s_dec[3];  // mirror0, mirror1, degrees
    const int tid = threadIdx.x;
    const int J = a.J, seg_len = a.obs_len + a.pred_len, TF = frame_tile(J), ntiles = tiles(seg_len, J);
    const int64_t b = blockIdx.x / ntiles;
    const int tile = (int)(blockIdx.x - b * ntiles);
    if (tid == 0) {
        const int64_t sidx = a.sample_idx[b];
        SampleDraw d;
        if (a.supplied) {
            d.offset = a.d_offset[b];
            d.mirror0 = a.d_mirror[2 * b] != 0;
            d.mirror1 = a.d_mirror[2 * b + 1] != 0;
            const int g = a.d_degrees[b];
            d.degrees = g < 0 ? -1 : g % 360;
        } else {
            d = draw_sample(a.seed, (uint64_t)sidx, a.epoch, a.augmentation, a.p_mirror, a.p_rot);
        }
        const int64_t seg = segment_index(sidx, a.stride, a.augmentation, d.offset, a.nseg);
        s_first = clamp_first(a.seg_first[seg], a.total_frames, seg_len);
        s_dec[0] = a.train ? d.mirror0 : 0;
        s_dec[1] = a.train ? d.mirror1 : 0;
        s_dec[2] = a.train ? d.degrees : -1;
        if (tile == 0) a.segment_idx[b] = seg;
    }
    __syncthreads();
    const int t0 = tile * TF, n = min(TF, seg_len - t0);
    load_span(a.frames + raw_frame(s_first, J, t0), n * 3 * J, raw, tid);
    __syncthreads();

    const int m0 = s_dec[0], m1 = s_dec[1], deg = s_dec[2];
    float c = 1.f, s = 0.f;
    if (deg >= 0) {
        c = a.rot[deg];
        s = a.rot[360 + deg];
    }
    const uint64_t row = (uint64_t)a.sample_idx[b];
    for (int i = tid; i < n * (J - 1); i += kThreads) {
        const int tl = i / (J - 1), j = 1 + (i - tl * (J - 1)), t = t0 + tl;
        const float* f = raw + lds_raw(J, tl);
        float x = f[3 * j], y = f[3 * j + 1], z = f[3 * j + 2];
        float hx = f[0], hy = f[1], hz = f[2];
        if (a.noisy && t < a.obs_len) {  // joints 1.. of the observation; the hip is never noised
            if (a.supplied) {
                const int64_t p = noise_pair(b, a.obs_len, J, t, j);
                if (a.d_mask[p]) {
                    x = x + a.d_noise[3 * p];
                    y = y + a.d_noise[3 * p + 1];
                    z = z + a.d_noise[3 * p + 2];
                }
            } else {
                float nx, ny, nz;
                if (draw_noise(a.seed, row, a.epoch, J, t, j, a.noise_level, a.noise_std, nx, ny, nz)) {
                    x = x + nx;
                    y = y + ny;
                    z = z + nz;
                }
            }
        }
        if (m0) {
            x = -x;
            hx = -hx;
        }
        if (m1) {
            y = -y;
            hy = -hy;
        }
        if (deg >= 0) {
            const float xr = c * x - s * y, yr = s * x + c * y;
            const float hxr = c * hx - s * hy, hyr = s * hx + c * hy;
            x = xr;
            y = yr;
            hx = hxr;
            hy = hyr;
        }
        if (a.repr != kVanilla) {
            x = x - hx;
            y = y - hy;
            z = z - hz;
            if (a.repr == kRescalePose) {
                x = x / a.box;
                y = y / a.box;
                z = z / a.box;
            }
        }
        float* o = outb + lds_out(J, tl) + 3 * (j - 1);
        o[0] = x;
        o[1] = y;
        o[2] = z;
    }
    __syncthreads();
    const int n_obs = obs_frames_in_tile(t0, n, a.obs_len);
    if (n_obs > 0) store_span(a.obs + out_frame(b, a.obs_len, J, t0), outb + lds_out(J, 0), n_obs * 3 * (J - 1), tid);
    if (n_obs < n)
        store_span(a.pred + out_frame(b, a.pred_len, J, t0 + n_obs - a.obs_len), outb + lds_out(J, n_obs),
                   (n - n_obs) * 3 * (J - 1), tid);
}

struct DrawArgs {
    const int64_t* sample_idx;
    int J, obs_len;
    int64_t augmentation;
    float p_mirror, p_rot;
    float noise_level, noise_std;
    uint64_t seed; int epoch;
    int32_t* offset; uint8_t* mirror; int32_t* degrees; uint8_t* mask; float* noise;
};

__global__ __launch_bounds__(kThreads) void k_motion_draws(DrawArgs a) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const uint64_t row = (uint64_t)a.sample_idx[b];
    if (tid == 0) {
        const SampleDraw d = draw_sample(a.seed, row, a.epoch, a.augmentation, a.p_mirror, a.p_rot);
        a.offset[b] = d.offset;
        a.mirror[2 * b] = (uint8_t)d.mirror0;
        a.mirror[2 * b + 1] = (uint8_t)d.mirror1;
        a.degrees[b] = d.degrees;
    }
    if (!a.mask) return;
    for (int i = tid; i < a.obs_len * (a.J - 1); i += kThreads) {
        const int t = i / (a.J - 1), j = 1 + (i - t * (a.J - 1));
        float nx, ny, nz;
        const bool hit = draw_noise(a.seed, row, a.epoch, a.J, t, j, a.noise_level, a.noise_std, nx, ny, nz);
        const int64_t p = noise_pair(b, a.obs_len, a.J, t, j);
        a.mask[p] = (uint8_t)hit;
        a.noise[3 * p] = nx;
        a.noise[3 * p + 1] = ny;
        a.noise[3 * p + 2] = nz;
    }
}

int bad(const char* fn, const char* what) { return set_error(SD_E_INVALID, std::string(fn) + ": " + what); }
int hip_fail(const char* what, hipError_t e) { return set_error(SD_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
bool prob_ok(float p) { return p >= 0.f && p <= 1.f; }  // false for NaN

}  // namespace

}  // namespace sd

extern "C" {

int32_t sd_motion_batch_frame_tile(int32_t joints) {
    if (joints < sd::motion::kMinJoints || joints > sd::motion::kMaxJoints) return -1;
    return sd::motion::frame_tile(joints);
}

int sd_motion_batch(const float* frames, int64_t total_frames, const int64_t* seg_first, int64_t nseg,
                    const int64_t* sample_idx, int64_t B, int32_t joints, int32_t obs_len, int32_t pred_len,
                    int64_t stride, int64_t augmentation, int32_t train, int32_t representation, float pose_box_size,
                    float da_mirroring, float da_rotations, int32_t noisy, float noise_level, float noise_std,
                    const float* rot_table, uint64_t seed, int32_t epoch, const int32_t* draw_offset,
                    const uint8_t* draw_mirror, const int32_t* draw_degrees, const uint8_t* draw_noise_mask,
                    const float* draw_noise, float* obs, float* pred, int64_t* segment_idx, void* stream) {
    using namespace sd;
    using namespace sd::motion;
    const char* fn = "motion_batch";
    if (B < 0) return bad(fn, "B must be >= 0");
    if (joints < kMinJoints || joints > kMaxJoints) return bad(fn, "joints must be in [2, 64]");
    if (obs_len < 1) return bad(fn, "obs_len must be >= 1");
    if (pred_len < 1) return bad(fn, "pred_len must be >= 1");
    if (obs_len > (1 << 20) || pred_len > (1 << 20)) return bad(fn, "obs_len and pred_len must be <= 2^20");
    if (nseg < 1) return bad(fn, "nseg must be >= 1");
    if (total_frames < (int64_t)obs_len + pred_len) return bad(fn, "total_frames must hold one segment (obs_len + pred_len)");
    if (stride < 1) return bad(fn, "stride must be >= 1");
    if (augmentation < 0) return bad(fn, "augmentation must be >= 0");
    if (augmentation > (1 << 30)) return bad(fn, "augmentation must be <= 2^30");
    if (representation != SD_MOTION_VANILLA && representation != SD_MOTION_CENTER_POSE && representation != SD_MOTION_RESCALE_POSE)
        return bad(fn, "representation must be SD_MOTION_VANILLA, SD_MOTION_CENTER_POSE or SD_MOTION_RESCALE_POSE");
    if (!(pose_box_size > 0.f)) return bad(fn, "pose_box_size must be > 0");
    if (!prob_ok(da_mirroring)) return bad(fn, "da_mirroring must be in [0, 1]");
    if (!prob_ok(da_rotations)) return bad(fn, "da_rotations must be in [0, 1]");
    if (!prob_ok(noise_level)) return bad(fn, "noise_level must be in [0, 1]");
    if (!(noise_std >= 0.f)) return bad(fn, "noise_std must be >= 0");
    if (B == 0) return SD_OK;
    if (!frames) return bad(fn, "frames is null");
    if (!seg_first) return bad(fn, "seg_first is null");
    if (!sample_idx) return bad(fn, "sample_idx is null");
    if (!rot_table) return bad(fn, "rot_table is null");
    if (!obs) return bad(fn, "obs is null");
    if (!pred) return bad(fn, "pred is null");
    if (!segment_idx) return bad(fn, "segment_idx is null");
    const bool supplied = draw_offset || draw_mirror || draw_degrees || draw_noise_mask || draw_noise;
    if (supplied) {
        if (!draw_offset) return bad(fn, "draw_offset is null (supplied draws come together)");
        if (!draw_mirror) return bad(fn, "draw_mirror is null (supplied draws come together)");
        if (!draw_degrees) return bad(fn, "draw_degrees is null (supplied draws come together)");
        if (noisy && !draw_noise_mask) return bad(fn, "draw_noise_mask is null (noisy observation, supplied draws)");
        if (noisy && !draw_noise) return bad(fn, "draw_noise is null (noisy observation, supplied draws)");
    }
    const int64_t nt = tiles(obs_len + pred_len, joints);
    if (B > INT32_MAX / nt) return bad(fn, "B times the tiles per sample exceeds 2^31 - 1 workgroups");
    MotionArgs a;
    a.frames = frames; a.total_frames = total_frames; a.seg_first = seg_first; a.nseg = nseg; a.sample_idx = sample_idx;
    a.J = joints; a.obs_len = obs_len; a.pred_len = pred_len; a.stride = stride; a.augmentation = augmentation;
    a.train = train != 0; a.repr = representation; a.box = pose_box_size; a.p_mirror = da_mirroring; a.p_rot = da_rotations;
    a.noisy = noisy != 0; a.noise_level = noise_level; a.noise_std = noise_std; a.rot = rot_table; a.seed = seed; a.epoch = epoch;
    a.supplied = supplied; a.d_offset = draw_offset; a.d_mirror = draw_mirror; a.d_degrees = draw_degrees;
    a.d_mask = draw_noise_mask; a.d_noise = draw_noise; a.obs = obs; a.pred = pred; a.segment_idx = segment_idx;
    hipLaunchKernelGGL(k_motion_batch, dim3((unsigned)(B * nt)), dim3(kThreads), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("motion_batch", e);
}

int sd_motion_draws(const int64_t* sample_idx, int64_t B, int32_t joints, int32_t obs_len, int64_t augmentation,
                    float da_mirroring, float da_rotations, float noise_level, float noise_std, uint64_t seed,
                    int32_t epoch, int32_t* offset, uint8_t* mirror, int32_t* degrees, uint8_t* noise_mask, float* noise,
                    void* stream) {
    using namespace sd;
    using namespace sd::motion;
    const char* fn = "motion_draws";
    if (B < 0) return bad(fn, "B must be >= 0");
    if (joints < kMinJoints || joints > kMaxJoints) return bad(fn, "joints must be in [2, 64]");
    if (obs_len < 1) return bad(fn, "obs_len must be >= 1");
    if (obs_len > (1 << 20)) return bad(fn, "obs_len must be <= 2^20");
    if (augmentation < 0) return bad(fn, "augmentation must be >= 0");
    if (augmentation > (1 << 30)) return bad(fn, "augmentation must be <= 2^30");
    if (!prob_ok(da_mirroring)) return bad(fn, "da_mirroring must be in [0, 1]");
    if (!prob_ok(da_rotations)) return bad(fn, "da_rotations must be in [0, 1]");
    if (!prob_ok(noise_level)) return bad(fn, "noise_level must be in [0, 1]");
    if (!(noise_std >= 0.f)) return bad(fn, "noise_std must be >= 0");
    if (B == 0) return SD_OK;
    if (B > INT32_MAX) return bad(fn, "B exceeds 2^31 - 1 workgroups");
    if (!sample_idx) return bad(fn, "sample_idx is null");
    if (!offset) return bad(fn, "offset is null");
    if (!mirror) return bad(fn, "mirror is null");
    if (!degrees) return bad(fn, "degrees is null");
    if ((noise_mask == nullptr) != (noise == nullptr)) return bad(fn, "noise_mask and noise come together (both or neither)");
    DrawArgs a;
    a.sample_idx = sample_idx; a.J = joints; a.obs_len = obs_len; a.augmentation = augmentation; a.p_mirror = da_mirroring;
    a.p_rot = da_rotations; a.noise_level = noise_level; a.noise_std = noise_std; a.seed = seed; a.epoch = epoch;
    a.offset = offset; a.mirror = mirror; a.degrees = degrees; a.mask = noise_mask; a.noise = noise;
    hipLaunchKernelGGL(k_motion_draws, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("motion_draws", e);
}

}  // extern "C"
