// Body-realism, limb-angle and motion-profile metrics on the device: the reference's
//   limb_stretching_normed_rmse / _mean, limb_jitter_normed_rmse / _mean   body_realism.py:109-199
//   mae (limb-angle error, with if_return_cossim)                          multimodal.py:76-102
//   motion_for_cmd                                                         cmd.py:10-12
// from one read of pred (B, S, T, J, 3).  Three kernels:
//   k_realism_target   one workgroup per sequence: the ground truth's mean limb lengths (f64) and,
//                      for the angles, its pair cosines and their acos (f64);
//   k_realism_pred     one workgroup per (sequence, sample): frames staged tile by tile into LDS with
//                      16-byte loads; limb lengths, pair cosines and joint steps of a tile are formed by
//                      all threads, then summed over the frames by one thread per limb / frame;
//   k_realism_reduce   one workgroup per sequence: the means over (S, L) from the f64 per-limb
//                      scratch, the minimum over samples of the angle errors, the motion profile's
//                      mean over samples.
// Every offset and LDS index comes from sd_realism_addr.h (also walked by the host emulation).
//
// Precision.  Limb lengths, their deviations from the ground truth's mean and all sums are f64: the
// stretch mean is |sum_t (ll_t - gt)| / T / gt, a difference of nearly equal lengths.
// Joint steps of the motion profile are f32 norms (relative error 1e-7) summed in f64.
//
// Summation order.  A limb's sums run over the frames in frame order in one thread; a sample's mean
// over limbs in limb order; a frame's motion over the joints in joint order; the angle errors of
// (frame, pair) item i = frame_in_tile * P + pair go to thread i % 256, are added there in item and
// tile order, and the 256 threads meet in an xor butterfly and as (w0 + w1) + (w2 + w3).  None of it
// depends on the sample index, the alignment of the sample's block or the grid, and contraction is
// off, so every instantiation of the kernel rounds alike.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_realism_addr.h"

namespace sd {

namespace {

using namespace realism;

// limb and angle-pair tables, passed by value (kernel arguments): limb l joins joints la[l], lb[l];
// pair p compares limbs pa[p], pb[p].  Unused entries are 0.
struct RealismTables {
    uint8_t la[kMaxLimbs], lb[kMaxLimbs], pa[kMaxPairs], pb[kMaxPairs];
};

// f64 length of joint a - joint b of one frame (f: the frame's 3 J floats)
__device__ __forceinline__ double limb_length(const float* f, int a, int b) {
    const double dx = (double)f[3 * a] - (double)f[3 * b], dy = (double)f[3 * a + 1] - (double)f[3 * b + 1],
                 dz = (double)f[3 * a + 2] - (double)f[3 * b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// cosine between two limbs of one frame (multimodal.py:77-82): the limb vectors run from the joint of
// lower index to the one of higher index (the sorted limbseq of :86); the denominator is clamped at 1e-7
__device__ __forceinline__ double pair_cos(const float* f, int a0, int a1, int b0, int b1) {
    const int alo = min(a0, a1), ahi = max(a0, a1), blo = min(b0, b1), bhi = max(b0, b1);
    const double ax = (double)f[3 * ahi] - (double)f[3 * alo], ay = (double)f[3 * ahi + 1] - (double)f[3 * alo + 1],
                 az = (double)f[3 * ahi + 2] - (double)f[3 * alo + 2];
    const double bx = (double)f[3 * bhi] - (double)f[3 * blo], by = (double)f[3 * bhi + 1] - (double)f[3 * blo + 1],
                 bz = (double)f[3 * bhi + 2] - (double)f[3 * blo + 2];
    const double dot = (ax * bx + ay * by) + az * bz;
    const double na = sqrt((ax * ax + ay * ay) + az * az), nb = sqrt((bx * bx + by * by) + bz * bz);
    const double den = na * nb;
    return dot / (den < 1e-7 ? 1e-7 : den);
}

__device__ __forceinline__ double clamped_acos(double c) { return acos(fmin(fmax(c, -1.0), 1.0)); }

// ---- ground truth ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_realism_target(const float* __restrict__ target, int T, int J, int L,
                                                             int P, RealismTables tab,
                                                             double* __restrict__ gt_len, double* __restrict__ gt_cos,
                                                             double* __restrict__ gt_ang) {
    __shared__ double ll[kMaxTile * kMaxLimbs];
    __shared__ uint8_t la[kMaxLimbs], lb[kMaxLimbs], pa[kMaxPairs], pb[kMaxPairs];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < kMaxLimbs) {
        la[tid] = tab.la[tid];
        lb[tid] = tab.lb[tid];
        pa[tid] = tab.pa[tid];
        pb[tid] = tab.pb[tid];
    }
    __syncthreads();
    double sum = 0.0;
    for (int t0 = 0; t0 < T; t0 += kMaxTile) {
        const int n = min(kMaxTile, T - t0);
        for (int i = tid; i < n * L; i += kThreads) {
            const int tl = i / L, l = i - tl * L;
            ll[i] = limb_length(target + target_frame(b, T, J, t0 + tl), la[l], lb[l]);
        }
        __syncthreads();
        if (tid < L)
            for (int tl = 0; tl < n; ++tl) sum += ll[tl * L + tid];
        __syncthreads();
    }
    if (tid < L) gt_len[gt_len_index(b, L, tid)] = sum / (double)T;
    if (gt_cos) {
        for (int i = tid; i < T * P; i += kThreads) {  // T * P <= 2^31 - 1 (checked on the host)
            const int t = i / P, p = i - t * P;
            const int a = pa[p], c = pb[p];
            const double cs = pair_cos(target + target_frame(b, T, J, t), la[a], lb[a], la[c], lb[c]);
            gt_cos[gt_pair_index(b, T, t, P, p)] = cs;
            if (gt_ang) gt_ang[gt_pair_index(b, T, t, P, p)] = clamped_acos(cs);
        }
    }
}

// ---- predictions -----------------------------------------------------------------------------------
// n frames from t0 on of the sample's block into the frame slots 1..n: 16-byte loads from the span's
// first 16-byte boundary on, never outside the span
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int N, float* __restrict__ dst, int tid) {
    int head, quads;
    stage_split((uint64_t)(uintptr_t)src, N, head, quads);
    for (int e = tid; e < head; e += kThreads) dst[e] = src[e];
    const float4* sq = reinterpret_cast<const float4*>(src + head);
    for (int q = tid; q < quads; q += kThreads) {
        const float4 v = sq[q];
        float* d = dst + head + 4 * q;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst[e] = src[e];
}

template <bool ANGLES, bool MOTION>
__global__ __launch_bounds__(kThreads) void k_realism_pred(
    const float* __restrict__ pred, int64_t BS, int S, int T, int J, int L, int P, RealismTables tab,
    const double* __restrict__ gt_len, const double* __restrict__ gt_cos, const double* __restrict__ gt_ang,
    float* __restrict__ none_out, float* __restrict__ persample_out, double* __restrict__ limb_scratch,
    float* __restrict__ ang_ps, float* __restrict__ cos_ps, float* __restrict__ motion_scratch) {
    extern __shared__ double dyn_lds[];
    __shared__ double q6[kQuantities * kMaxLimbs];
    __shared__ double wsum[8];
    __shared__ uint8_t la[kMaxLimbs], lb[kMaxLimbs], pa[kMaxPairs], pb[kMaxPairs];
    double* ll = dyn_lds;
    float* fr = reinterpret_cast<float*>(dyn_lds + lds_ll_doubles(J, L));
    float* mb = fr + lds_frame_floats(J);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TF = frame_tile(J), J3 = 3 * J;
    const int64_t w = blockIdx.x, b = w / S;
    if (tid < kMaxLimbs) {
        la[tid] = tab.la[tid];
        lb[tid] = tab.lb[tid];
        pa[tid] = tab.pa[tid];
        pb[tid] = tab.pb[tid];
    }
    const double gt = tid < L ? gt_len[gt_len_index(b, L, tid)] : 1.0;
    double s1 = 0.0, s2 = 0.0, j1 = 0.0, j2 = 0.0, prev = 0.0;  // thread l < L: limb l's sums over the frames
    double acc_a = 0.0, acc_c = 0.0;                             // this thread's share of the angle errors
    const bool want_acos = ANGLES && ang_ps != nullptr;
    __syncthreads();

    for (int t0 = 0; t0 < T; t0 += TF) {
        const int n = min(TF, T - t0);
        stage_tile(pred + pred_frame(w, T, J, t0), n * J3, fr + lds_slot(J, 1), tid);
        __syncthreads();
        for (int i = tid; i < n * L; i += kThreads) {
            const int tl = i / L, l = i - tl * L;
            ll[i] = limb_length(fr + lds_slot(J, tl + 1), la[l], lb[l]);
        }
        if (MOTION) {
            for (int i = tid; i < n * J; i += kThreads) {
                const int tl = i / J, j = i - tl * J;
                if (t0 + tl == 0) continue;  // the first frame has no step
                const float* c = fr + lds_slot(J, tl + 1) + 3 * j;
                const float* q = fr + lds_slot(J, tl) + 3 * j;
                const float dx = c[0] - q[0], dy = c[1] - q[1], dz = c[2] - q[2];
                mb[i] = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            }
        }
        if (ANGLES) {
            for (int i = tid; i < n * P; i += kThreads) {
                const int tl = i / P, p = i - tl * P;
                const int a = pa[p], c = pb[p];
                const double cs = pair_cos(fr + lds_slot(J, tl + 1), la[a], lb[a], la[c], lb[c]);
                const int64_t g = gt_pair_index(b, T, t0 + tl, P, p);
                acc_c += fabs(cs - gt_cos[g]);
                if (want_acos) acc_a += fabs(clamped_acos(cs) - gt_ang[g]);
            }
        }
        __syncthreads();
        if (tid < L) {
            for (int tl = 0; tl < n; ++tl) {
                const double x = ll[tl * L + tid], dev = x - gt;
                s1 += dev;
                s2 += dev * dev;
                if (t0 + tl > 0) {
                    const double d = fabs(x - prev);
                    j1 += d;
                    j2 += d * d;
                }
                prev = x;
            }
        } else if (MOTION && tid >= kMotionLane0 && tid < kMotionLane0 + n) {
            const int tl = tid - kMotionLane0, t = t0 + tl;
            if (t > 0) {
                double m = 0.0;
                for (int j = 0; j < J; ++j) m += (double)mb[tl * J + j];
                motion_scratch[motion_index(w, T, t)] = (float)(m / (double)J);
            }
        } else if (MOTION && tid >= kCarryLane0) {  // the tile's last frame is the next tile's slot 0
            for (int e = tid - kCarryLane0; e < J3; e += kThreads - kCarryLane0)
                fr[lds_slot(J, 0) + e] = fr[lds_slot(J, n) + e];
        }
        __syncthreads();
    }

    if (tid < L) {
        const double dT = (double)T, dT1 = (double)(T - 1);  // T == 1: 0 / 0 = NaN jitter, as the reference
        const double v[kQuantities] = {sqrt(s2 / dT) / gt, (s2 / dT) / gt,    sqrt(j2 / dT1) / gt,
                                       (j2 / dT1) / gt,    fabs(s1 / dT) / gt, (j1 / dT1) / gt};
#pragma unroll
        for (int q = 0; q < kQuantities; ++q) {
            const int64_t o = limb_index(q, BS, w, L, tid);
            if (none_out) none_out[o] = (float)v[q];
            if (limb_scratch) limb_scratch[o] = v[q];
            q6[q * kMaxLimbs + tid] = v[q];
        }
    }
    if (ANGLES) {
        for (int o = 32; o > 0; o >>= 1) {
            acc_a += __shfl_xor(acc_a, o);
            acc_c += __shfl_xor(acc_c, o);
        }
        if (lane == 0) {
            wsum[wave] = acc_a;
            wsum[4 + wave] = acc_c;
        }
    }
    __syncthreads();
    if (persample_out && tid < kQuantities) {
        double a = 0.0;
        for (int l = 0; l < L; ++l) a += q6[tid * kMaxLimbs + l];
        persample_out[persample_index(tid, BS, w)] = (float)(a / (double)L);
    }
    if (ANGLES && tid == kMotionLane0) {
        const double items = (double)T * (double)P, deg = 180.0 / 3.14159265358979323846;
        if (ang_ps) ang_ps[w] = (float)(((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) / items * deg);
        if (cos_ps) cos_ps[w] = (float)(((wsum[4] + wsum[5]) + (wsum[6] + wsum[7])) / items * deg);
    }
}

// ---- per sequence: means over (S, L), minimum over samples, motion profile ----------------------------
// (the minimum over samples: min_or_nan, sd_internal.h)
__global__ __launch_bounds__(kThreads) void k_realism_reduce(int64_t B, int S, int T, int L,
                                                             const double* __restrict__ limb_scratch,
                                                             float* __restrict__ mean_out,
                                                             const float* __restrict__ ang_ps, float* __restrict__ ang_min,
                                                             const float* __restrict__ cos_ps, float* __restrict__ cos_min,
                                                             const float* __restrict__ motion_scratch,
                                                             float* __restrict__ motion_out) {
    __shared__ double rows[kQuantities * kMaxSamples];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, BS = B * S;
    if (mean_out) {
        for (int i = tid; i < kQuantities * S; i += kThreads) {
            const int q = i / S, s = i - q * S;
            double a = 0.0;
            for (int l = 0; l < L; ++l) a += limb_scratch[limb_index(q, BS, b * S + s, L, l)];
            rows[q * kMaxSamples + s] = a;
        }
    }
    __syncthreads();
    if (mean_out && tid < kQuantities) {
        double a = 0.0;
        for (int s = 0; s < S; ++s) a += rows[tid * kMaxSamples + s];
        mean_out[mean_index(tid, B, b)] = (float)(a / ((double)S * (double)L));
    }
    if (ang_min && tid == 64) ang_min[b] = min_or_nan(ang_ps + b * S, S);
    if (cos_min && tid == 128) cos_min[b] = min_or_nan(cos_ps + b * S, S);
    if (motion_out) {
        for (int t = 1 + tid; t < T; t += kThreads) {
            double a = 0.0;
            for (int s = 0; s < S; ++s) a += (double)motion_scratch[motion_index(b * S + s, T, t)];
            motion_out[motion_index(b, T, t)] = (float)(a / (double)S);
        }
    }
}

// the tables of a call, validated (0 on success, else the message is set)
int make_tables(const char* who, int32_t joints, const int32_t* limbseq, int32_t nlimbs, const int32_t* angle_pairs,
                int32_t npairs, RealismTables& tab) {
    const std::string w(who);
    if (joints < 1 || joints > kMaxJoints) return set_error(SD_E_INVALID, w + ": joints must be in 1..64");
    if (nlimbs < 1 || nlimbs > kMaxLimbs) return set_error(SD_E_INVALID, w + ": nlimbs must be in 1..64");
    if (npairs < 0 || npairs > kMaxPairs) return set_error(SD_E_INVALID, w + ": npairs must be in 0..64");
    if (!limbseq) return set_error(SD_E_INVALID, w + ": limbseq is null");
    if (npairs > 0 && !angle_pairs) return set_error(SD_E_INVALID, w + ": angle_pairs is null");
    tab = RealismTables{};
    for (int l = 0; l < nlimbs; ++l) {
        const int32_t a = limbseq[2 * l], b = limbseq[2 * l + 1];
        if (a < 0 || a >= joints || b < 0 || b >= joints)
            return set_error(SD_E_INVALID, w + ": limbseq[" + std::to_string(l) + "] has a joint outside [0, joints)");
        tab.la[l] = (uint8_t)a;
        tab.lb[l] = (uint8_t)b;
    }
    for (int p = 0; p < npairs; ++p) {
        const int32_t a = angle_pairs[2 * p], b = angle_pairs[2 * p + 1];
        if (a < 0 || a >= nlimbs || b < 0 || b >= nlimbs)
            return set_error(SD_E_INVALID, w + ": angle_pairs[" + std::to_string(p) + "] has a limb outside [0, nlimbs)");
        tab.pa[p] = (uint8_t)a;
        tab.pb[p] = (uint8_t)b;
    }
    return SD_OK;
}

int hip_fail(const char* what, hipError_t e) {
    return set_error(SD_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

}  // namespace sd

extern "C" {

int32_t sd_realism_frame_tile(int32_t joints) {
    if (joints < 1 || joints > sd::realism::kMaxJoints) return sd::set_error(SD_E_INVALID, "realism: joints must be in 1..64");
    return sd::realism::frame_tile(joints);
}

int sd_realism_target(const float* target, int64_t nseq, int32_t frames, int32_t joints, const int32_t* limbseq,
                      int32_t nlimbs, const int32_t* angle_pairs, int32_t npairs, double* gt_len_mean, double* gt_cos,
                      double* gt_ang, void* stream) {
    using namespace sd;
    if (nseq < 0 || nseq > INT32_MAX) return set_error(SD_E_INVALID, "realism_target: nseq must be in 0..2^31-1");
    if (frames < 1) return set_error(SD_E_INVALID, "realism_target: frames must be >= 1");
    RealismTables tab;
    if (int rc = make_tables("realism_target", joints, limbseq, nlimbs, angle_pairs, npairs, tab)) return rc;
    if ((gt_cos || gt_ang) && npairs < 1)
        return set_error(SD_E_INVALID, "realism_target: npairs must be >= 1 when gt_cos / gt_ang are asked for");
    if (gt_ang && !gt_cos) return set_error(SD_E_INVALID, "realism_target: gt_ang needs gt_cos");
    if ((int64_t)frames * std::max(npairs, nlimbs) > INT32_MAX)
        return set_error(SD_E_INVALID, "realism_target: frames * max(nlimbs, npairs) must be below 2^31");
    if (nseq == 0) return SD_OK;
    if (!target) return set_error(SD_E_INVALID, "realism_target: target is null");
    if (!gt_len_mean) return set_error(SD_E_INVALID, "realism_target: gt_len_mean is null");
    hipLaunchKernelGGL(k_realism_target, dim3((unsigned)nseq), dim3(realism::kThreads), 0, (hipStream_t)stream, target,
                       frames, joints, nlimbs, npairs, tab, gt_len_mean, gt_cos, gt_ang);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_realism_target", e);
}

int sd_realism(const float* pred, int64_t nseq, int32_t samples, int32_t frames, int32_t joints, const int32_t* limbseq,
               int32_t nlimbs, const int32_t* angle_pairs, int32_t npairs, const double* gt_len_mean,
               const double* gt_cos, const double* gt_ang, int32_t target_frames, float* none_out, float* persample_out,
               double* limb_scratch, float* mean_out, float* angle_persample, float* cossim_persample, float* angle_min,
               float* cossim_min, float* motion_scratch, float* motion_out, void* stream) {
    using namespace sd;
    if (nseq < 0) return set_error(SD_E_INVALID, "realism: nseq must be >= 0");
    if (samples < 1 || samples > realism::kMaxSamples) return set_error(SD_E_INVALID, "realism: samples must be in 1..64");
    if (frames < 1) return set_error(SD_E_INVALID, "realism: frames must be >= 1");
    RealismTables tab;
    if (int rc = make_tables("realism", joints, limbseq, nlimbs, angle_pairs, npairs, tab)) return rc;
    const bool angles = angle_persample || cossim_persample || angle_min || cossim_min;
    if (angles && target_frames != frames)
        return set_error(SD_E_INVALID, "realism: target_frames must equal frames when angle outputs are asked for");
    if (angles && npairs < 1) return set_error(SD_E_INVALID, "realism: npairs must be >= 1 when angle outputs are asked for");
    if (nseq * samples > INT32_MAX) return set_error(SD_E_INVALID, "realism: nseq * samples must be below 2^31");
    if ((int64_t)frames * std::max(npairs, nlimbs) > INT32_MAX)
        return set_error(SD_E_INVALID, "realism: frames * max(nlimbs, npairs) must be below 2^31");
    if (nseq == 0) return SD_OK;
    if (!pred) return set_error(SD_E_INVALID, "realism: pred is null");
    if (!gt_len_mean) return set_error(SD_E_INVALID, "realism: gt_len_mean is null");
    if (angles && !gt_cos) return set_error(SD_E_INVALID, "realism: gt_cos is null");
    if ((angle_persample || angle_min) && !gt_ang) return set_error(SD_E_INVALID, "realism: gt_ang is null");
    if (mean_out && !limb_scratch) return set_error(SD_E_INVALID, "realism: mean_out needs limb_scratch");
    if (angle_min && !angle_persample) return set_error(SD_E_INVALID, "realism: angle_min needs angle_persample");
    if (cossim_min && !cossim_persample) return set_error(SD_E_INVALID, "realism: cossim_min needs cossim_persample");
    if (motion_out && !motion_scratch) return set_error(SD_E_INVALID, "realism: motion_out needs motion_scratch");
    const bool motion = motion_scratch && frames > 1;
    if (!motion) motion_out = nullptr;  // frames == 1: an empty profile

    const hipStream_t s = (hipStream_t)stream;
    const int64_t BS = nseq * samples;
    const dim3 grid((unsigned)BS), block(realism::kThreads);
    const size_t lds = realism::lds_bytes(joints, nlimbs);
#define SD_REALISM_LAUNCH(A, M)                                                                                      \
    hipLaunchKernelGGL((k_realism_pred<A, M>), grid, block, lds, s, pred, BS, samples, frames, joints, nlimbs, npairs, \
                       tab, gt_len_mean, gt_cos, gt_ang, none_out, persample_out, limb_scratch, angle_persample,     \
                       cossim_persample, motion_scratch)
    if (angles && motion) SD_REALISM_LAUNCH(true, true);
    else if (angles) SD_REALISM_LAUNCH(true, false);
    else if (motion) SD_REALISM_LAUNCH(false, true);
    else SD_REALISM_LAUNCH(false, false);
#undef SD_REALISM_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("k_realism_pred", e);
    if (mean_out || angle_min || cossim_min || motion_out) {
        hipLaunchKernelGGL(k_realism_reduce, dim3((unsigned)nseq), block, 0, s, nseq, samples, frames, nlimbs,
                           limb_scratch, mean_out, angle_persample, angle_min, cossim_persample, cossim_min,
                           motion_scratch, motion_out);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("k_realism_reduce", e);
    }
    return SD_OK;
}

}  // extern "C"
