// On-device evaluation metrics over the sampler's outputs ("next" #2): the
// reference's multimodal metrics computed where the latents already are, one workgroup per
// sequence, fixed summation order (deterministic).
//   pairwise: mean over the sample pairs i < j of the L1 (lat_apd, multimodal.py:137-151) and
//             L2 (apd, multimodal.py:15-35) distances between the flattened samples;
//   ade / fde: per sample the mean over frames (ade, multimodal.py:44-57) or the last frame
//             (fde, :60-73) of the L2 distance to the target, then the minimum over samples;
//   mmade / mmfde: the same minimum against each of a sequence's multimodal ground truths,
//             averaged over them (multimodal.py:108-135): one workgroup per (sequence, gt) pair,
//             then a fixed-order mean per sequence.
//             Non-finite values go where torch takes them: the minimum over samples is torch.min's, NaN
//             as soon as one sample's distance is NaN (min_or_nan, sd_internal.h; a +Inf distance loses
//             to any number), and the means over pairs and over ground truths propagate NaN.
//   best sample: per (sequence, sample) the mean per-joint L2 distance to the target (mpjpe,
//             multimodal.py:37-42), one workgroup per pair; then per sequence the first minimum and
//             the gather of that sample (metrics/utils.py:12-30) -- see k_sample_dist below.
// Samples are (S, X) rows of one sequence, X = T_frames * F (flattened frame-major, as
// `pred.reshape(batch, n_samples, seq_length, -1)`).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"

namespace sd {

namespace {

constexpr int kMaxSamples = 64;
constexpr int kChunk = 64;  // features staged per step

// pair p (0 <= p < S(S-1)/2) -> (i, j), i < j, row-major over the upper triangle
__device__ __forceinline__ void pair_of(int p, int S, int& i, int& j) {
    int r = 0, base = 0;
    while (base + (S - 1 - r) <= p) {
        base += S - 1 - r;
        ++r;
    }
    i = r;
    j = r + 1 + (p - base);
}

__global__ __launch_bounds__(256) void k_pairwise(const float* __restrict__ x, int S, int64_t X,
                                                  float* __restrict__ l1_mean, float* __restrict__ l2_mean) {
    __shared__ float tile[kMaxSamples * kChunk];
    __shared__ float red1[kMaxSamples * (kMaxSamples - 1) / 2];
    __shared__ float red2[kMaxSamples * (kMaxSamples - 1) / 2];
    const int tid = threadIdx.x;
    const int P = S * (S - 1) / 2;
    const float* xs = x + (int64_t)blockIdx.x * S * X;
    constexpr int PPT = (kMaxSamples * (kMaxSamples - 1) / 2 + 255) / 256;  // pairs per thread
    float s1[PPT], s2[PPT];
    int pi[PPT], pj[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        s1[k] = s2[k] = 0.f;
        const int p = tid + 256 * k;
        pi[k] = pj[k] = 0;
        if (p < P) pair_of(p, S, pi[k], pj[k]);
    }
    for (int64_t f0 = 0; f0 < X; f0 += kChunk) {
        const int n = (int)min((int64_t)kChunk, X - f0);
        __syncthreads();
        for (int e = tid; e < S * kChunk; e += 256) {
            const int s = e / kChunk, f = e - s * kChunk;
            tile[e] = f < n ? xs[(int64_t)s * X + f0 + f] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            if (tid + 256 * k >= P) continue;
            const float* a = tile + pi[k] * kChunk;
            const float* b = tile + pj[k] * kChunk;
            float t1 = 0.f, t2 = 0.f;
            for (int f = 0; f < kChunk; ++f) {
                const float d = a[f] - b[f];
                t1 += fabsf(d);
                t2 = fmaf(d, d, t2);
            }
            s1[k] += t1;
            s2[k] += t2;
        }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = tid + 256 * k;
        if (p < P) {
            red1[p] = s1[k];
            red2[p] = sqrtf(s2[k]);
        }
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int p = 0; p < P; ++p) {
            a += red1[p];
            b += red2[p];
        }
        if (l1_mean) l1_mean[blockIdx.x] = (float)(a / P);
        if (l2_mean) l2_mean[blockIdx.x] = (float)(b / P);
    }
}

// pred (S, T, F) per sequence, target (T, F): per sample mean_t ||pred - target|| (ade) and the
// last frame's distance (fde), minimum over samples
// pair_seq (nullable): workgroup b compares target b with pred sequence pair_seq[b] (mm metrics)
__global__ __launch_bounds__(256) void k_ade_fde(const float* __restrict__ pred, const float* __restrict__ target,
                                                 int S, int T, int64_t F, float* __restrict__ ade,
                                                 float* __restrict__ fde, float* __restrict__ per_sample_ade,
                                                 float* __restrict__ per_sample_fde,
                                                 const int64_t* __restrict__ pair_seq) {
    __shared__ float mean_t[kMaxSamples], last_t[kMaxSamples];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seq = pair_seq ? pair_seq[blockIdx.x] : (int64_t)blockIdx.x;
    const float* ps = pred + seq * S * T * F;
    const float* tg = target + (int64_t)blockIdx.x * T * F;
    for (int s = wave; s < S; s += 4) {
        float acc_t = 0.f, last = 0.f;
        for (int t = 0; t < T; ++t) {
            float d2 = 0.f;
            for (int64_t f = lane; f < F; f += 64) {
                const float d = ps[((int64_t)s * T + t) * F + f] - tg[(int64_t)t * F + f];
                d2 = fmaf(d, d, d2);
            }
            for (int o = 32; o > 0; o >>= 1) d2 += __shfl_xor(d2, o);
            const float dn = sqrtf(d2);
            acc_t += dn;
            if (t == T - 1) last = dn;
        }
        if (lane == 0) {
            mean_t[s] = acc_t / T;
            last_t[s] = last;
        }
    }
    __syncthreads();
    if (per_sample_ade)
        for (int s = tid; s < S; s += 256) per_sample_ade[(int64_t)blockIdx.x * S + s] = mean_t[s];
    if (per_sample_fde)
        for (int s = tid; s < S; s += 256) per_sample_fde[(int64_t)blockIdx.x * S + s] = last_t[s];
    // the reference's dist.min(axis=-1).values (multimodal.py:55, :71, :117, :133): a NaN sample makes the minimum NaN
    if (ade && tid == 0) ade[blockIdx.x] = min_or_nan(mean_t, S);
    if (fde && tid == 64) fde[blockIdx.x] = min_or_nan(last_t, S);
}

// per sequence the mean of its pairs' values in pair order (offsets: nseq + 1); 0 pairs -> NaN
// (the mean of an empty tensor, as torch)
__global__ __launch_bounds__(256) void k_segment_mean(const float* __restrict__ v, const int64_t* __restrict__ off,
                                                      int64_t nseq, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nseq) return;
    const int64_t a = off[i], b = off[i + 1];
    float acc = 0.f;
    for (int64_t k = a; k < b; ++k) acc += v[k];
    out[i] = b > a ? acc / (float)(b - a) : __builtin_nanf("");
}

// ---- best-of-k training relaxation (reference trainer.py:207-222, get_ksimilarity_loss) ----------
// Per sequence the index of the smallest similarity among its k samples -- torch.min(dim).indices:
// the first minimum, and the first NaN if there is one (torch's min propagates NaN) -- and the
// diffusion loss at that index (torch.gather).  sim == loss in the latent space.
__global__ __launch_bounds__(256) void k_best_of_k(const float* __restrict__ sim, const float* __restrict__ loss,
                                                   int64_t nseq, int k, int64_t* __restrict__ idx,
                                                   float* __restrict__ sel) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nseq) return;
    const float* v = sim + b * k;
    int best = 0;
    float bv = v[0];
    for (int j = 1; j < k; ++j) {
        const float x = v[j];
        if (bv != bv) break;                  // a NaN already selected: the first NaN wins
        if (x != x || x < bv) {
            best = j;
            bv = x;
        }
    }
    if (idx) idx[b] = best;
    if (sel) sel[b] = loss[b * k + best];
}

// gradient of the gather: d loss[b, j] = d sel[b] at j = idx[b], else 0
__global__ __launch_bounds__(256) void k_best_of_k_bwd(const float* __restrict__ dsel, const int64_t* __restrict__ idx,
                                                       int64_t nseq, int k, float* __restrict__ dloss) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nseq * k) return;
    const int64_t b = e / k;
    dloss[e] = (e - b * k == idx[b]) ? dsel[b] : 0.f;
}

// AutoEncoder.loss(pred, y, reduction='none') (reference autoencoder.py:80-98): per sample
// mean over frames of the mean over joints of the sum over coordinates of |d| (l1) or d^2 (mse);
// pred (nseq, S, T, J, C), target (nseq, T, J, C) (the future, not repeated).  One wave per
// (sequence, sample); frame sums in frame order.
__global__ __launch_bounds__(256) void k_pose_loss(const float* __restrict__ pred, const float* __restrict__ target,
                                                   int64_t nseq, int S, int T, int J, int C, int mse,
                                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nseq * S) return;  // wave-uniform
    const int64_t b = w / S;
    const int JC = J * C;
    const float* p = pred + w * (int64_t)T * JC;
    const float* tg = target + b * (int64_t)T * JC;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
        float fr = 0.f;  // sum over joints and coordinates of this frame
        for (int e = lane; e < JC; e += 64) {
            const float d = p[(int64_t)t * JC + e] - tg[(int64_t)t * JC + e];
            fr += mse ? d * d : fabsf(d);
        }
        for (int o = 32; o > 0; o >>= 1) fr += __shfl_xor(fr, o);
        acc += fr / (float)J;
    }
    if (lane == 0) out[w] = acc / (float)T;
}

// ---- best-sample selection (reference metrics/utils.py:12-30 choose_best_sample / get_best_sample_idx,
// multimodal.py:37-42 mpjpe, eval_utils.py:59-62 the long-term rollout's selection) -----------------
// d[b, s] = mean over frames and joints of ||pred[b, s, t, j, :] - target[b, t, j, :]||_2.
//
// Layout.  One workgroup per (sequence, sample) pair; a sample's block is N = T * J joints = L = 3 N
// floats.  The block is cut into groups of 4 joints (12 floats) by joint index alone: thread `tid`
// takes the groups tid, tid + 256, ...  A group is read with 16-byte loads: three when the block
// starts on a 16-byte boundary, else the four aligned quads that cover it (the block starts A = 1..3
// floats past a boundary; a group starts a multiple of 4 floats into the block, so A is the same for
// all of them).  A group whose quads would reach outside the block -- the first one of a misaligned
// block, the last one or two -- is read float by float.  pred and target have an A each.
//
// Summation order.  It depends on the joint index only, never on the alignment or the sample index:
// a joint's distance is sqrt(fma(dz, dz, fma(dy, dy, dx dx))); a group's four distances are added in
// joint order in f32; a thread adds its groups in f64 in group order; the 64 lanes' sums meet in an
// xor butterfly (f64) and the 4 waves' as (w0 + w1) + (w2 + w3).  So two samples with the same bytes
// get the same bits, and no f32 chain is longer than 4 terms.
template <int A>
__device__ __forceinline__ void load12(const float* __restrict__ blk, int64_t e0, int64_t L, float (&v)[12]) {
    constexpr int Q = A ? 4 : 3;
    const int64_t ws = e0 - A;  // on a 16-byte boundary (e0 % 4 == 0)
    if (ws >= 0 && ws + 4 * Q <= L) {
        const float4* q = reinterpret_cast<const float4*>(blk + ws);
        float w[4 * Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const float4 x = q[k];
            w[4 * k] = x.x;
            w[4 * k + 1] = x.y;
            w[4 * k + 2] = x.z;
            w[4 * k + 3] = x.w;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = w[i + A];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = e0 + i < L ? blk[e0 + i] : 0.f;
    }
}

__device__ __forceinline__ void load12(int A, const float* __restrict__ blk, int64_t e0, int64_t L, float (&v)[12]) {
    switch (A) {  // the same in every thread of the workgroup
        case 0: load12<0>(blk, e0, L, v); break;
        case 1: load12<1>(blk, e0, L, v); break;
        case 2: load12<2>(blk, e0, L, v); break;
        default: load12<3>(blk, e0, L, v); break;
    }
}

// floats past the previous 16-byte boundary (p is 4-byte aligned)
__device__ __forceinline__ int quad_phase(const float* p) { return (int)(((uintptr_t)p >> 2) & 3); }

__global__ __launch_bounds__(256) void k_sample_dist(const float* __restrict__ pred,
                                                     const float* __restrict__ target, int64_t pairs, int S,
                                                     int64_t N, float* __restrict__ d) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t L = 3 * N, groups = (N + 3) / 4;
    for (int64_t w = blockIdx.x; w < pairs; w += gridDim.x) {
        const float* p = pred + w * L;
        const float* tg = target + (w / S) * L;
        const int ap = quad_phase(p), at = quad_phase(tg);
        double acc = 0.0;
        for (int64_t g = tid; g < groups; g += 256) {
            float pv[12], tv[12];
            load12(ap, p, 12 * g, L, pv);
            load12(at, tg, 12 * g, L, tv);
            float s4 = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dx = pv[3 * k] - tv[3 * k], dy = pv[3 * k + 1] - tv[3 * k + 1],
                            dz = pv[3 * k + 2] - tv[3 * k + 2];
                const float dn = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
                if (4 * g + k < N) s4 += dn;
            }
            acc += (double)s4;
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (tid == 0) d[w] = (float)(((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) / (double)N);
        __syncthreads();
    }
}

// dst[0, n) = src[0, n) by the threads t0, t0 + nt, ...: 16-byte stores from dst's first 16-byte
// boundary on, fed by 16-byte loads where src is on a boundary there too, else by four floats
__device__ __forceinline__ void copy_span(float* __restrict__ dst, const float* __restrict__ src, int64_t n,
                                          int64_t t0, int64_t nt) {
    const int64_t head = min(n, (int64_t)((4 - quad_phase(dst)) & 3));
    const int64_t quads = (n - head) / 4;
    for (int64_t e = t0; e < head; e += nt) dst[e] = src[e];
    float4* dq = reinterpret_cast<float4*>(dst + head);
    if (quad_phase(src + head) == 0) {
        const float4* sq = reinterpret_cast<const float4*>(src + head);
        for (int64_t q = t0; q < quads; q += nt) dq[q] = sq[q];
    } else {
        for (int64_t q = t0; q < quads; q += nt) {
            const float* sp = src + head + 4 * q;
            dq[q] = make_float4(sp[0], sp[1], sp[2], sp[3]);
        }
    }
    for (int64_t e = head + 4 * quads + t0; e < n; e += nt) dst[e] = src[e];
}

// Per sequence the index of the smallest distance (torch.min(dim).indices as k_best_of_k: the first
// minimum, the first NaN if there is one), that distance, and the selected sample's block of L
// floats / its last Lt floats.  Workgroup (b, c): sequence b, share c of the copies; c = 0 writes
// the index and the distance.
__global__ __launch_bounds__(256) void k_best_select(const float* __restrict__ pred, const float* __restrict__ d,
                                                     int S, int64_t L, int64_t Lt, float* __restrict__ min_out,
                                                     int64_t* __restrict__ idx_out, float* __restrict__ best_out,
                                                     float* __restrict__ tail_out) {
    __shared__ float dv[kMaxSamples];
    __shared__ int sel;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (tid < S) dv[tid] = d[b * S + tid];
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        float bv = dv[0];
        for (int j = 1; j < S; ++j) {
            const float x = dv[j];
            if (bv != bv) break;  // a NaN already selected: the first NaN wins
            if (x != x || x < bv) {
                best = j;
                bv = x;
            }
        }
        sel = best;
        if (blockIdx.y == 0) {
            if (idx_out) idx_out[b] = best;
            if (min_out) min_out[b] = bv;
        }
    }
    __syncthreads();
    const float* src = pred + (b * S + sel) * L;
    const int64_t t0 = (int64_t)blockIdx.y * 256 + tid, nt = (int64_t)gridDim.y * 256;
    if (best_out) copy_span(best_out + b * L, src, L, t0, nt);
    if (tail_out) copy_span(tail_out + b * Lt, src + (L - Lt), Lt, t0, nt);
}

// Class-wise sums of the CMD (cmd.py:22-29): thread (c, w) goes on from sum[c, w] and adds values[r, w] of
// the rows r of class c in ascending row order, in float64: one chain per (class, column), so the state
// after a dataset does not depend on how its rows were cut into calls.  Thread (c, 0) counts the class's
// rows, thread (0, 0) the rows of the call (a class index outside [0, classes) counts there only).
__global__ __launch_bounds__(256) void k_class_sum(const float* __restrict__ values, const int64_t* __restrict__ cls,
                                                   int64_t rows, int width, int classes, double* __restrict__ sum,
                                                   int64_t* __restrict__ count, int64_t* __restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)classes * width) return;
    const int c = (int)(e / width), w = (int)(e - (int64_t)c * width);
    double acc = sum[e];
    int64_t n = 0;
    for (int64_t r = 0; r < rows; ++r)
        if (cls[r] == c) {
            acc += (double)values[r * width + w];
            ++n;
        }
    sum[e] = acc;
    if (w == 0) count[c] += n;
    if (e == 0) total[0] += rows;
}

}  // namespace

}  // namespace sd

// The entry points (include/skeldiff.h): argument checks, then the launches.
extern "C" {
using namespace sd;

int sd_pairwise_distances(const float* x, int64_t nseq, int32_t samples, int64_t features, float* l1_mean,
                          float* l2_mean, void* stream) {
    if (nseq < 0 || samples < 2 || samples > kMaxSamples || features < 1)
        return set_error(SD_E_INVALID, "pairwise distances: need 2..64 samples, features >= 1");
    if (nseq == 0) return SD_OK;
    if (!x) return set_error(SD_E_INVALID, "pairwise distances: null input");
    hipLaunchKernelGGL(k_pairwise, dim3((unsigned)nseq), dim3(256), 0, (hipStream_t)stream, x, samples, features, l1_mean,
                       l2_mean);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_ade_fde(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
               int64_t features, float* ade, float* fde, float* per_sample_ade, float* per_sample_fde, void* stream) {
    if (nseq < 0 || samples < 1 || samples > kMaxSamples || frames < 1 || features < 1)
        return set_error(SD_E_INVALID, "ade/fde: need 1..64 samples, frames >= 1, features >= 1");
    if (nseq == 0) return SD_OK;
    if (!pred || !target) return set_error(SD_E_INVALID, "ade/fde: null input");
    hipLaunchKernelGGL(k_ade_fde, dim3((unsigned)nseq), dim3(256), 0, (hipStream_t)stream, pred, target, samples, frames,
                       features, ade, fde, per_sample_ade, per_sample_fde, (const int64_t*)nullptr);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_mm_ade_fde(const float* pred, const float* gts, const int64_t* pair_seq, int64_t npairs,
                  const int64_t* seq_offsets, int64_t nseq, int32_t samples, int32_t frames, int64_t features,
                  float* pair_ade, float* pair_fde, float* mmade, float* mmfde, void* stream) {
    if (nseq < 0 || npairs < 0 || samples < 1 || samples > kMaxSamples || frames < 1 || features < 1)
        return set_error(SD_E_INVALID, "mmade/mmfde: need 1..64 samples, frames >= 1, features >= 1");
    if (nseq == 0) return SD_OK;
    if (!seq_offsets || (npairs > 0 && (!pred || !gts || !pair_seq)) || (mmade && !pair_ade) || (mmfde && !pair_fde))
        return set_error(SD_E_INVALID, "mmade/mmfde: null input (pair outputs are required for the means)");
    hipStream_t s = (hipStream_t)stream;
    if (npairs > 0)
        hipLaunchKernelGGL(k_ade_fde, dim3((unsigned)npairs), dim3(256), 0, s, pred, gts, samples, frames, features, pair_ade,
                           pair_fde, (float*)nullptr, (float*)nullptr, pair_seq);
    const dim3 g((unsigned)((nseq + 255) / 256));
    if (mmade) hipLaunchKernelGGL(k_segment_mean, g, dim3(256), 0, s, pair_ade, seq_offsets, nseq, mmade);
    if (mmfde) hipLaunchKernelGGL(k_segment_mean, g, dim3(256), 0, s, pair_fde, seq_offsets, nseq, mmfde);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// best-of-k training relaxation (trainer.py:182-222)
int sd_best_of_k(const float* sim, const float* loss, int64_t nseq, int32_t k, int64_t* idx_out, float* loss_out,
                 void* stream) {
    if (nseq < 0 || k < 1) return set_error(SD_E_INVALID, "best_of_k: nseq >= 0, k >= 1");
    if (nseq == 0) return SD_OK;
    if (!loss || (!idx_out && !loss_out)) return set_error(SD_E_INVALID, "best_of_k: null buffer");
    hipLaunchKernelGGL(k_best_of_k, dim3((unsigned)((nseq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       sim ? sim : loss, loss, nseq, k, idx_out, loss_out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_best_of_k_backward(const float* dloss_sel, const int64_t* idx, int64_t nseq, int32_t k, float* dloss,
                          void* stream) {
    if (nseq < 0 || k < 1) return set_error(SD_E_INVALID, "best_of_k_backward: nseq >= 0, k >= 1");
    if (nseq == 0) return SD_OK;
    if (!dloss_sel || !idx || !dloss) return set_error(SD_E_INVALID, "best_of_k_backward: null buffer");
    hipLaunchKernelGGL(k_best_of_k_bwd, dim3((unsigned)((nseq * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       dloss_sel, idx, nseq, k, dloss);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_pose_loss(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
                 int32_t joints, int32_t dims, int32_t mse, float* per_sample, void* stream) {
    if (nseq < 0 || samples < 1 || frames < 1 || joints < 1 || dims < 1)
        return set_error(SD_E_INVALID, "pose_loss: samples, frames, joints, dims >= 1");
    if (nseq == 0) return SD_OK;
    if (!pred || !target || !per_sample) return set_error(SD_E_INVALID, "pose_loss: null buffer");
    hipLaunchKernelGGL(k_pose_loss, dim3((unsigned)((nseq * samples + 3) / 4)), dim3(256), 0, (hipStream_t)stream, pred,
                       target, nseq, samples, frames, joints, dims, (int)(mse != 0), per_sample);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// best-sample selection (metrics/utils.py:12-30, multimodal.py:37-42): per (sequence, sample) the mean
// per-joint L2 distance to the target, then per sequence the first minimum, its distance and the
// gathered trajectory / its last tail_frames frames (each output but per_sample nullable)
int sd_best_sample(const float* pred, const float* target, int64_t nseq, int32_t samples, int32_t frames,
                   int32_t joints, int32_t coords, int32_t tail_frames, float* per_sample, float* min_out,
                   int64_t* idx_out, float* best_out, float* tail_out, void* stream) {
    if (nseq < 0 || nseq > INT32_MAX) return set_error(SD_E_INVALID, "best_sample: nseq must be in 0..2^31-1");
    if (samples < 1 || samples > kMaxSamples) return set_error(SD_E_INVALID, "best_sample: samples must be in 1..64");
    if (coords != 3) return set_error(SD_E_INVALID, "best_sample: coords must be 3");
    if (frames < 1) return set_error(SD_E_INVALID, "best_sample: frames must be >= 1");
    if (joints < 1) return set_error(SD_E_INVALID, "best_sample: joints must be >= 1");
    if (tail_frames < 0 || tail_frames > frames) return set_error(SD_E_INVALID, "best_sample: tail_frames must be in 0..frames");
    if (tail_out && tail_frames == 0) return set_error(SD_E_INVALID, "best_sample: tail_out given with tail_frames = 0");
    if (nseq == 0) return SD_OK;
    if (!pred) return set_error(SD_E_INVALID, "best_sample: pred is null");
    if (!target) return set_error(SD_E_INVALID, "best_sample: target is null");
    if (!per_sample) return set_error(SD_E_INVALID, "best_sample: per_sample is required (it is the workspace)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t pairs = nseq * samples, N = (int64_t)frames * joints, L = 3 * N, Lt = 3 * (int64_t)tail_frames * joints;
    hipLaunchKernelGGL(k_sample_dist, dim3((unsigned)std::min(pairs, (int64_t)1 << 30)), dim3(256), 0, s, pred, target, pairs,
                       samples, N, per_sample);
    if (min_out || idx_out || best_out || tail_out) {
        // 2 quads per thread and share; the copies of one sequence are at most a few hundred KB
        const int64_t span = std::max(best_out ? L : (int64_t)0, tail_out ? Lt : (int64_t)0);
        const unsigned shares = (unsigned)std::min(std::max((span + 2047) / 2048, (int64_t)1), (int64_t)32);
        hipLaunchKernelGGL(k_best_select, dim3((unsigned)nseq, shares), dim3(256), 0, s, pred, per_sample, samples, L, Lt,
                           min_out, idx_out, best_out, tail_out);
    }
    SD_HIP(hipGetLastError());
    return SD_OK;
}

// class-wise CMD accumulation (cmd.py:17-29): the state (sum, count, total) is updated in place
int sd_class_sum(const float* values, const int64_t* cls, int64_t rows, int32_t width, int32_t classes, double* sum,
                 int64_t* count, int64_t* total, void* stream) {
    if (rows < 0) return set_error(SD_E_INVALID, "class_sum: rows must be >= 0");
    if (width < 1) return set_error(SD_E_INVALID, "class_sum: width must be >= 1");
    if (classes < 1) return set_error(SD_E_INVALID, "class_sum: classes must be >= 1");
    if (rows == 0) return SD_OK;
    if (!values) return set_error(SD_E_INVALID, "class_sum: values is null");
    if (!cls) return set_error(SD_E_INVALID, "class_sum: cls is null");
    if (!sum) return set_error(SD_E_INVALID, "class_sum: sum is null");
    if (!count) return set_error(SD_E_INVALID, "class_sum: count is null");
    if (!total) return set_error(SD_E_INVALID, "class_sum: total is null");
    const int64_t cells = (int64_t)classes * width;
    hipLaunchKernelGGL(k_class_sum, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values, cls, rows,
                       (int)width, (int)classes, sum, count, total);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // extern "C"
