// Validation metrics of the two training loops on the device: the reference's
//   limb_length_variance / _jitter / _error / _variation_difference_wrtGT   body_realism.py:4-107
//   MeanPerJointPositionError, FinalDisplacementError (streamed)            ignite_mpjpe.py, ignite_fde.py
// Three kernels:
//   k_limb_stats    one workgroup per (sequence, sample): frames staged tile by tile into LDS with
//                   16-byte loads (the body-realism pass's staging); the limb lengths of a tile (and the
//                   target's) are formed by all threads in f64, then one thread per limb folds the tile
//                   into the limb's variance state, jitter sum / maximum / minimum and error sum; at the
//                   end the reductions over the limbs;
//   k_limb_reduce   one workgroup per sequence: the reductions over the samples, from the f64 scratch;
//   k_frame_error   one workgroup per 16 (frame, joint) cells of the window: 16 rows at a time are staged
//                   and their per-joint distances formed by all threads, then one thread per cell adds
//                   them, in row order, onto the f64 sum it holds.
// Every offset, LDS index and thread role comes from sd_validation_addr.h (also walked by the host emulation).
//
// Precision.  Limb lengths and everything made of them are f64; results are rounded to f32 once.  The
// variance over the frames is never E[x^2] - mean^2 of raw lengths: a tile's sum of squares is taken about
// the tile's own mean (two passes over the staged lengths) and tiles are joined by Chan's combine step
// (validation::var_combine).  The per-joint distance of the frame error is an f64 norm of f64 differences.
//
// Summation order.  A limb's sums run over the frames in frame order in one thread; a sample's reductions
// over the limbs in limb order, a sequence's over the samples in sample order.  A (frame, joint) cell of the
// frame error adds its rows in ascending row order onto the value the state holds, so the state is bitwise
// the same however the rows were split into calls.  No atomics; contraction is off; nothing depends on the
// alignment of a block (staging only copies).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_device.h"
#include "sd_internal.h"
#include "sd_validation_addr.h"

namespace sd {

namespace {

using namespace validation;

// the limb table, passed by value (a kernel argument): limb l joins joints la[l], lb[l]
struct LimbTable {
    uint8_t la[kMaxLimbs], lb[kMaxLimbs];
};

// f64 length of joint a - joint b of one frame (f: the frame's 3 J floats)
__device__ __forceinline__ double limb_length(const float* f, int a, int b) {
    const double dx = (double)f[3 * a] - (double)f[3 * b], dy = (double)f[3 * a + 1] - (double)f[3 * b + 1],
                 dz = (double)f[3 * a + 2] - (double)f[3 * b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ double fold(int op, double acc, double x) {
    return op == 0 ? acc + x : (op == 1 ? max_keep_nan(acc, x) : min_keep_nan(acc, x));
}

// N floats from src into LDS: 16-byte loads from the span's first 16-byte boundary on, never outside it
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int N, float* __restrict__ dst, int tid) {
    int head, quads;
    stage_split((uint64_t)(uintptr_t)src, N, head, quads);
    for (int e = tid; e < head; e += kThreads) dst[e] = src[e];
    for (int q = tid; q < quads; q += kThreads) {
        const floatx4 v = ld4(src + head + 4 * q);
        float* d = dst + head + 4 * q;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst[e] = src[e];
}

// ---- limb statistics -------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_limb_stats(const float* __restrict__ pred, const float* __restrict__ target,
                                                         int64_t BS, int S, int T, int J, int L, LimbTable tab,
                                                         float* __restrict__ limb_out, float* __restrict__ sample_out,
                                                         double* __restrict__ sample_scratch,
                                                         float* __restrict__ steps_out,
                                                         float* __restrict__ steps_diff_out) {
    extern __shared__ double dyn_lds[];
    __shared__ double q5[kStats * kMaxLimbs];
    __shared__ uint8_t la[kMaxLimbs], lb[kMaxLimbs];
    double* ll = dyn_lds;
    double* tl = dyn_lds + lds_len_doubles(J, L);
    float* fr = reinterpret_cast<float*>(dyn_lds + 2 * lds_len_doubles(J, L));

    const int tid = threadIdx.x;
    const int TF = frame_tile(J), J3 = 3 * J;
    const int64_t w = blockIdx.x, b = w / S;
    if (tid < kMaxLimbs) {
        la[tid] = tab.la[tid];
        lb[tid] = tab.lb[tid];
    }
    // thread l < L: limb l's state over the frames
    double cn = 0.0, cmean = 0.0, cm2 = 0.0;  // frames so far, their mean length, sum (x - mean)^2
    double j1 = 0.0, jmax = 0.0, jmin = 0.0, e1 = 0.0, prev = 0.0, tprev = 0.0;
    __syncthreads();

    for (int t0 = 0; t0 < T; t0 += TF) {
        const int n = min(TF, T - t0);
        stage_tile(pred + pred_frame(w, T, J, t0), n * J3, fr, tid);
        __syncthreads();
        for (int i = tid; i < n * L; i += kThreads) {
            const int f = i / L, l = i - f * L;
            ll[i] = limb_length(fr + f * J3, la[l], lb[l]);
            if (target) tl[i] = limb_length(target + target_frame(b, T, J, t0 + f), la[l], lb[l]);
        }
        __syncthreads();
        if (tid < L) {
            double sm = 0.0;
            for (int f = 0; f < n; ++f) sm += ll[f * L + tid];
            const double tmean = sm / (double)n;
            double tm2 = 0.0;
            for (int f = 0; f < n; ++f) {
                const double d = ll[f * L + tid] - tmean;
                tm2 += d * d;
            }
            var_combine(cn, cmean, cm2, (double)n, tmean, tm2);
            for (int f = 0; f < n; ++f) {
                const double x = ll[f * L + tid];
                const int t = t0 + f;
                if (t > 0) {
                    const double d = fabs(x - prev);
                    j1 += d;
                    jmax = t == 1 ? d : max_keep_nan(jmax, d);
                    jmin = t == 1 ? d : min_keep_nan(jmin, d);
                    if (steps_out) steps_out[step_index(w, T, t, L, tid)] = (float)d;
                    if (steps_diff_out)
                        steps_diff_out[step_index(w, T, t, L, tid)] = (float)(d - fabs(tl[f * L + tid] - tprev));
                }
                prev = x;
                if (target) {
                    tprev = tl[f * L + tid];
                    e1 += fabs(tprev - x);
                }
            }
        }
        __syncthreads();
    }

    if (tid < L) {
        const double nan = __builtin_nan("");
        const double dT1 = (double)(T - 1);  // T == 1: 0 / 0 = NaN variance and jitter mean, as the reference
        const double v[kStats] = {cm2 / dT1, j1 / dT1, T > 1 ? jmax : nan, T > 1 ? jmin : nan,
                                  target ? e1 / (double)T : nan};
#pragma unroll
        for (int q = 0; q < kStats; ++q) {
            if (limb_out) limb_out[limb_index(q, BS, w, L, tid)] = (float)v[q];
            q5[q * kMaxLimbs + tid] = v[q];
        }
    }
    __syncthreads();
    if ((sample_out || sample_scratch) && tid < kSampleRows) {
        const int op = sample_row_op(tid);
        const double* src = q5 + sample_row_stat(tid) * kMaxLimbs;
        double a = src[0];
        for (int l = 1; l < L; ++l) a = fold(op, a, src[l]);
        if (op == 0) a /= (double)L;
        if (sample_out) sample_out[sample_index(tid, BS, w)] = (float)a;
        if (sample_scratch) sample_scratch[sample_index(tid, BS, w)] = a;
    }
}

__global__ __launch_bounds__(64) void k_limb_reduce(int64_t B, int S, const double* __restrict__ sample_scratch,
                                                    float* __restrict__ seq_out) {
    const int r = threadIdx.x;
    const int64_t b = blockIdx.x, BS = B * S;
    if (r >= kSeqRows) return;
    const int op = seq_row_op(r), src = seq_row_source(r);
    double a = sample_scratch[sample_index(src, BS, b * S)];
    for (int s = 1; s < S; ++s) a = fold(op, a, sample_scratch[sample_index(src, BS, b * S + s)]);
    if (op == 0) a /= (double)S;
    seq_out[seq_index(r, B, b)] = (float)a;
}

// ---- streaming frame error -------------------------------------------------------------------------
// one row's span of N floats into its LDS slot, by the row's kCells lanes
__device__ __forceinline__ void stage_span(const float* __restrict__ src, int N, float* __restrict__ dst, int k) {
    int head, quads, quad, scalar;
    stage_split((uint64_t)(uintptr_t)src, N, head, quads);
    span_lane(k, N, head, quads, quad, scalar);
    if (quad >= 0) {
        const floatx4 v = ld4(src + head + 4 * quad);
        float* d = dst + head + 4 * quad;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    if (scalar >= 0) dst[scalar] = src[scalar];
}

__global__ __launch_bounds__(kThreads) void k_frame_error(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const int64_t* __restrict__ idx, int64_t rows, int S, int T,
                                                          int J, int frame0, int nframes, double* __restrict__ sum,
                                                          int64_t* __restrict__ count) {
    __shared__ float ps[kRows * kSpanFloats], ts[kRows * kSpanFloats];
    __shared__ double en[kRows * kCells];
    const int tid = threadIdx.x, pr = tid / kCells, k = tid - pr * kCells;
    const int64_t cells = cell_count(nframes, J), c0 = (int64_t)blockIdx.x * kCells;
    const int nc = cells_of_block(cells, blockIdx.x), N = 3 * nc;
    double acc = tid < nc ? sum[c0 + tid] : 0.0;
    for (int64_t r0 = 0; r0 < rows; r0 += kRows) {
        const int nr = (int)(rows - r0 < kRows ? rows - r0 : kRows);
        int s = -1;
        if (pr < nr) {
            const int64_t r = r0 + pr;
            s = idx ? sample_or_none(idx[r], S) : 0;
            if (s >= 0) stage_span(pred + pred_span(r, s, S, T, J, frame0, c0), N, ps + lds_span(pr, 0), k);
            stage_span(target + target_span(r, T, J, frame0, c0), N, ts + lds_span(pr, 0), k);
        }
        __syncthreads();
        if (pr < nr && k < nc) {
            double e = __builtin_nan("");
            if (s >= 0) {
                const float* p = ps + lds_span(pr, 3 * k);
                const float* g = ts + lds_span(pr, 3 * k);
                const double dx = (double)p[0] - (double)g[0], dy = (double)p[1] - (double)g[1],
                             dz = (double)p[2] - (double)g[2];
                e = sqrt((dx * dx + dy * dy) + dz * dz);
            }
            en[lds_cell(pr, k)] = e;
        }
        __syncthreads();
        if (tid < nc)
            for (int i = 0; i < nr; ++i) acc += en[lds_cell(i, tid)];
        // no barrier here: the next pass rewrites ps / ts, last read before the barrier above, and
        // rewrites en only after its own first barrier, which these readers of en reach first
    }
    if (tid < nc) sum[c0 + tid] = acc;
    if (blockIdx.x == 0 && tid == 0) count[0] += rows;
}

int make_table(const char* who, int32_t joints, const int32_t* limbseq, int32_t nlimbs, LimbTable& tab) {
    const std::string w(who);
    if (joints < 1 || joints > kMaxJoints) return set_error(SD_E_INVALID, w + ": joints must be in 1..64");
    if (nlimbs < 1 || nlimbs > kMaxLimbs) return set_error(SD_E_INVALID, w + ": nlimbs must be in 1..64");
    if (!limbseq) return set_error(SD_E_INVALID, w + ": limbseq is null");
    tab = LimbTable{};
    for (int l = 0; l < nlimbs; ++l) {
        const int32_t a = limbseq[2 * l], b = limbseq[2 * l + 1];
        if (a < 0 || a >= joints || b < 0 || b >= joints)
            return set_error(SD_E_INVALID, w + ": limbseq[" + std::to_string(l) + "] has a joint outside [0, joints)");
        tab.la[l] = (uint8_t)a;
        tab.lb[l] = (uint8_t)b;
    }
    return SD_OK;
}

int hip_fail(const char* what, hipError_t e) {
    return set_error(SD_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

}  // namespace sd

extern "C" {

int sd_limb_stats(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames, int32_t joints,
                  const int32_t* limbseq, int32_t nlimbs, float* limb_out, float* sample_out, double* sample_scratch,
                  float* seq_out, float* steps_out, float* steps_diff_out, void* stream) {
    using namespace sd;
    if (nseq < 0) return set_error(SD_E_INVALID, "limb_stats: nseq must be >= 0");
    if (samples < 1 || samples > validation::kMaxSamples) return set_error(SD_E_INVALID, "limb_stats: samples must be in 1..64");
    if (frames < 1) return set_error(SD_E_INVALID, "limb_stats: frames must be >= 1");
    LimbTable tab;
    if (int rc = make_table("limb_stats", joints, limbseq, nlimbs, tab)) return rc;
    if (nseq * samples > INT32_MAX) return set_error(SD_E_INVALID, "limb_stats: nseq * samples must be below 2^31");
    if ((int64_t)frames * nlimbs > INT32_MAX) return set_error(SD_E_INVALID, "limb_stats: frames * nlimbs must be below 2^31");
    if (seq_out && !sample_scratch) return set_error(SD_E_INVALID, "limb_stats: seq_out needs sample_scratch");
    if (steps_diff_out && !target) return set_error(SD_E_INVALID, "limb_stats: steps_diff_out needs target");
    if (nseq == 0) return SD_OK;
    if (!pred) return set_error(SD_E_INVALID, "limb_stats: pred is null");
    if (!limb_out && !sample_out && !sample_scratch && !steps_out && !steps_diff_out) return SD_OK;  // nothing asked for

    const hipStream_t s = (hipStream_t)stream;
    const int64_t BS = nseq * samples;
    hipLaunchKernelGGL(k_limb_stats, dim3((unsigned)BS), dim3(validation::kThreads), validation::limb_lds_bytes(joints, nlimbs),
                       s, pred, target, BS, samples, frames, joints, nlimbs, tab, limb_out, sample_out, sample_scratch,
                       frames > 1 ? steps_out : nullptr, frames > 1 ? steps_diff_out : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("k_limb_stats", e);
    if (seq_out) {
        hipLaunchKernelGGL(k_limb_reduce, dim3((unsigned)nseq), dim3(64), 0, s, nseq, samples, sample_scratch, seq_out);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail("k_limb_reduce", e);
    }
    return SD_OK;
}

int sd_frame_error_update(const float* pred, const float* target, const int64_t* idx, int64_t rows, int32_t samples,
                          int32_t frames, int32_t joints, int32_t frame0, int32_t nframes, double* sum, int64_t* count,
                          void* stream) {
    using namespace sd;
    if (rows < 0) return set_error(SD_E_INVALID, "frame_error_update: rows must be >= 0");
    if (samples < 1 || samples > validation::kMaxSamples)
        return set_error(SD_E_INVALID, "frame_error_update: samples must be in 1..64");
    if (!idx && samples != 1) return set_error(SD_E_INVALID, "frame_error_update: idx is null, which needs samples == 1");
    if (frames < 1) return set_error(SD_E_INVALID, "frame_error_update: frames must be >= 1");
    if (joints < 1 || joints > validation::kMaxJoints)
        return set_error(SD_E_INVALID, "frame_error_update: joints must be in 1..64");
    if (frame0 < 0 || frame0 >= frames) return set_error(SD_E_INVALID, "frame_error_update: frame0 must be in [0, frames)");
    if (nframes < 1 || nframes > frames - frame0)
        return set_error(SD_E_INVALID, "frame_error_update: nframes must be in 1..frames - frame0");
    if (!sum) return set_error(SD_E_INVALID, "frame_error_update: sum is null");
    if (!count) return set_error(SD_E_INVALID, "frame_error_update: count is null");
    if (rows == 0) return SD_OK;
    if (!pred) return set_error(SD_E_INVALID, "frame_error_update: pred is null");
    if (!target) return set_error(SD_E_INVALID, "frame_error_update: target is null");
    const int64_t cells = validation::cell_count(nframes, joints);
    const int64_t blocks = (cells + validation::kCells - 1) / validation::kCells;
    if (blocks > INT32_MAX) return set_error(SD_E_INVALID, "frame_error_update: nframes * joints must be below 2^35");
    hipLaunchKernelGGL(k_frame_error, dim3((unsigned)blocks), dim3(validation::kThreads), 0, (hipStream_t)stream, pred,
                       target, idx, rows, samples, frames, joints, frame0, nframes, sum, count);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_frame_error", e);
}

}  // extern "C"
