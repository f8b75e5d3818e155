// Address arithmetic of the body-realism kernels (sd_realism.hip), as host + device functions: the
// kernels take every global offset, LDS index and loop bound from here, and so does the stand-alone
// host emulation (tests/host/realism_emulation.cpp), which walks every workgroup x thread x load /
// store with the same functions and checks each against the size of the buffer it goes to.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_RHD __host__ __device__ inline
#else
#define SD_RHD inline
#endif

namespace sd {
namespace realism {

constexpr int kThreads = 256;       // threads of every workgroup here
constexpr int kMaxSamples = 64, kMaxJoints = 64, kMaxLimbs = 64, kMaxPairs = 64;
constexpr int kStageFloats = 2048;  // floats of pred one frame tile stages (8 KB)
constexpr int kMaxTile = 32;        // frames per tile at most: one thread per frame sums the motion
constexpr int kQuantities = 6;      // srmse_std, srmse_var, jrmse_std, jrmse_var, smean, jmean
constexpr int kMotionLane0 = 64;    // first thread of the per-frame motion sums (limbs: 0..63)
constexpr int kCarryLane0 = 128;    // first thread of the copy of a tile's last frame to slot 0

// frames staged per tile: a function of the joint count alone (10 for J = 64, 13 for J = 51, 32 up to J = 21)
SD_RHD int frame_tile(int J) {
    const int t = kStageFloats / (3 * J);
    return t > kMaxTile ? kMaxTile : (t < 1 ? 1 : t);
}

// ---- global offsets (elements) -----------------------------------------------------------------
// first float of frame t of sample w (= sequence * S + sample) in pred (B, S, T, J, 3)
SD_RHD int64_t pred_frame(int64_t w, int T, int J, int t) { return (w * T + t) * (int64_t)(3 * J); }
// first float of frame t of sequence b in target (B, T, J, 3)
SD_RHD int64_t target_frame(int64_t b, int T, int J, int t) { return (b * T + t) * (int64_t)(3 * J); }
// a span of N floats at byte address `addr` (4-byte aligned): [0, head) float by float, `quads`
// 16-byte loads from its first 16-byte boundary on, then [head + 4 quads, N) float by float
SD_RHD void stage_split(uint64_t addr, int N, int& head, int& quads) {
    const int to_boundary = (int)((4 - ((addr >> 2) & 3)) & 3);
    head = to_boundary < N ? to_boundary : N;
    quads = (N - head) / 4;
}
SD_RHD int64_t gt_len_index(int64_t b, int L, int l) { return b * L + l; }                     // (B, L)
SD_RHD int64_t gt_pair_index(int64_t b, int T, int t, int P, int p) { return (b * T + t) * P + p; }  // (B, T, P)
// quantity q of limb l of sample w in the (6, B * S, L) arrays (`none` outputs and the f64 scratch)
SD_RHD int64_t limb_index(int q, int64_t BS, int64_t w, int L, int l) { return ((int64_t)q * BS + w) * L + l; }
SD_RHD int64_t persample_index(int q, int64_t BS, int64_t w) { return (int64_t)q * BS + w; }    // (6, B * S)
SD_RHD int64_t mean_index(int q, int64_t B, int64_t b) { return (int64_t)q * B + b; }           // (6, B)
// step t - 1 -> t (1 <= t < T) of sample w in the motion scratch (B * S, T - 1); of sequence b in (B, T - 1)
SD_RHD int64_t motion_index(int64_t w, int T, int t) { return w * (int64_t)(T - 1) + (t - 1); }

// ---- dynamic LDS of the prediction pass ----------------------------------------------------------
// doubles ll[tile][L] first, then floats: frames[(tile + 1)][3 J] (slot 0 = the frame before the
// tile, slot 1 + i = frame i of the tile), then motion[tile][J]
SD_RHD int lds_ll_doubles(int J, int L) { return frame_tile(J) * L; }
SD_RHD int lds_frame_floats(int J) { return (frame_tile(J) + 1) * 3 * J; }
SD_RHD int lds_motion_floats(int J) { return frame_tile(J) * J; }
SD_RHD size_t lds_bytes(int J, int L) {
    return sizeof(double) * (size_t)lds_ll_doubles(J, L) + sizeof(float) * (size_t)(lds_frame_floats(J) + lds_motion_floats(J));
}
SD_RHD int lds_slot(int J, int slot) { return slot * 3 * J; }  // first float of a frame slot

}  // namespace realism
}  // namespace sd
