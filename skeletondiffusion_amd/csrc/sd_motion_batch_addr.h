// Address arithmetic and the random-draw map of the motion-batch kernels (sd_motion_batch.hip), as
// host + device functions: the kernels take every global offset, LDS index and loop bound from here,
// and so does the stand-alone host emulation (tests/host/motion_batch_emulation.cpp), which walks
// every workgroup x thread x load / store with the same functions and checks each against the size
// of the buffer it goes to.
//
// Philox quad map (key = seed, row = sample_idx, step = epoch; philox_at in sd_philox.h).  u(w) is
// u01(w) = ((w >> 8) + 0.5) 2^-24.
//   quad 0   .x  offset  = (int)(x % (2 A + 1)) - A            (A = augmentation; 0 when A == 0)
//            .y  mirror axis 0 when u(y) < da_mirroring
//            .z  mirror axis 1 when u(z) < da_mirroring
//            .w  rotate when u(w) < da_rotations
//   quad 1   .x  degrees = x % 360                             (used when quad 0 says rotate)
//   quad 2 + t (J - 1) + (j - 1), observation frame t, joint j >= 1:
//            (x, y) -> box_muller -> the normals of coordinates 0 and 1
//            (z, w) -> box_muller -> its first normal is coordinate 2 (the second is not used)
//            the pair is hit when u(m) < noise_level, m = the low bytes of x, y, z, w from bit 0 up
//            (x & 255) | (y & 255) << 8 | (z & 255) << 16 | (w & 255) << 24: box_muller reads bits
//            8..31 of a word only, so the mask is independent of the three normals
//   noise element = noise_std * normal, one f32 multiplication.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_MHD __host__ __device__ inline
#else
#define SD_MHD inline
#endif

namespace sd {
namespace motion {

constexpr int kThreads = 256;       // threads of every workgroup here
constexpr int kMinJoints = 2, kMaxJoints = 64;
constexpr int kStageFloats = 2048;  // floats of raw frames one tile stages (8 KB); as many again for its output
constexpr int kMaxTile = 32;        // frames per tile at most
constexpr uint32_t kQuadSample = 0, kQuadDegrees = 1, kQuadNoise0 = 2;

// representations (include/skeldiff.h SD_MOTION_*)
constexpr int kVanilla = 0, kCenterPose = 1, kRescalePose = 2;

// frames per tile: a function of the joint count alone (10 for J = 64, 13 for J = 52, 31 for J = 22, 32 up to J = 21)
SD_MHD int frame_tile(int J) {
    const int t = kStageFloats / (3 * J);
    return t > kMaxTile ? kMaxTile : (t < 1 ? 1 : t);
}
SD_MHD int tiles(int seg_len, int J) { return (seg_len + frame_tile(J) - 1) / frame_tile(J); }

// segment of a sample (base_dataset.py:110-113); always clamped, so the table read stays in bounds
SD_MHD int64_t segment_index(int64_t sample_idx, int64_t stride, int64_t augmentation, int64_t offset, int64_t nseg) {
    int64_t s = stride * sample_idx + augmentation;
    if (augmentation != 0) s += offset;
    return s < 0 ? 0 : (s > nseg - 1 ? nseg - 1 : s);
}
// first global frame of a segment, kept inside the resident frames whatever the table holds
SD_MHD int64_t clamp_first(int64_t first, int64_t total_frames, int seg_len) {
    const int64_t hi = total_frames - seg_len;
    return first < 0 ? 0 : (first > hi ? hi : first);
}

// ---- global offsets (elements) -----------------------------------------------------------------
// first float of frame t of the segment that starts at global frame `first` in frames (F, J, 3)
SD_MHD int64_t raw_frame(int64_t first, int J, int t) { return (first + t) * (int64_t)(3 * J); }
// first float of frame t of sample b in obs / pred (B, len, J - 1, 3)
SD_MHD int64_t out_frame(int64_t b, int len, int J, int t) { return (b * len + t) * (int64_t)(3 * (J - 1)); }
// (frame t, joint j >= 1) of sample b in noise_mask (B, obs, J - 1); times 3 in noise (B, obs, J - 1, 3)
SD_MHD int64_t noise_pair(int64_t b, int obs_len, int J, int t, int j) { return (b * obs_len + t) * (int64_t)(J - 1) + (j - 1); }
SD_MHD uint32_t noise_quad(int J, int t, int j) { return kQuadNoise0 + (uint32_t)t * (uint32_t)(J - 1) + (uint32_t)(j - 1); }
// a span of N floats at byte address `addr` (4-byte aligned): [0, head) float by float, `quads`
// 16-byte accesses from its first 16-byte boundary on, then [head + 4 quads, N) float by float
SD_MHD void span_split(uint64_t addr, int N, int& head, int& quads) {
    const int to_boundary = (int)((4 - ((addr >> 2) & 3)) & 3);
    head = to_boundary < N ? to_boundary : N;
    quads = (N - head) / 4;
}
// frames [t0, t0 + n) of a segment: the first n_obs of them go to obs, the rest to pred
SD_MHD int obs_frames_in_tile(int t0, int n, int obs_len) {
    const int k = obs_len - t0;
    return k < 0 ? 0 : (k > n ? n : k);
}

// ---- LDS (floats) ------------------------------------------------------------------------------
// raw[kStageFloats]: frame i of the tile at i * 3 J;  outb[kStageFloats]: its output at i * 3 (J - 1)
SD_MHD int lds_raw(int J, int i) { return i * 3 * J; }
SD_MHD int lds_out(int J, int i) { return i * 3 * (J - 1); }

}  // namespace motion
}  // namespace sd
