// Diversity ranking on the device: the reference's find_samples_maxapd_wrtGT and
// get_closest_and_nfurthest_maxapd (src/metrics/ranking.py:3-63) pick, per sequence, the samples that are
// mutually most distant with a batched torch.cdist and a Python loop with .tolist() / .nonzero() round
// trips per pick.  Here:
//   k_rank_dist    phase 1: per sequence the distance matrix of its points P_0 = target, P_{1+s} = sample s
//                  (N = samples + 1), in tiles of 32 x 32; only the tile pairs ti <= tj run, one 64-thread
//                  workgroup each, 4 x 4 entries per thread; an entry i < j is stored at (i, j) and (j, i).
//                  No pair of two sequences is ever formed.
//   k_rank_select  phase 2: one 256-thread workgroup per sequence, thread i holds m_i; the closest sample
//                  (from_closest) and every pick are an arg-min / arg-max over the workgroup on a fixed xor
//                  butterfly per wave and the four waves in order (sd_rank_addr.h).  No atomics.
//
// The value of an entry is sd_cdist's (include/skeldiff.h, sd_mmgt.hip): features in chunks of 32 from
// feature 0 on, t = fma(d_k, d_k, t) for k ascending inside a chunk, acc = acc + t in chunk order, then the
// correctly rounded square root.  It is a function of the two rows and `features` only, so with
// from_closest the matrix of [sample c; samples] needs no second pass: its row 0 is row 1 + c of the matrix
// of [target; samples].
//
// LDS layout of phase 1 (k_cdist's, at a quarter of the tile): a chunk of a row tile is float4 = four
// consecutive features of one row at slot [k quad][row]; thread (tx, ty) owns rows ty + 8 i and columns
// 4 tx + j (i, j < 4); the column operand's row `col` lies at slot (col & 3) * 8 + (col >> 2), so the eight
// distinct slots a wave reads per operand are consecutive; the k-quad stride is padded by two slots.  The
// roles and slots are sd_rank_addr.h's functions, which tests/host/rank_emulation.cpp walks on the host.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_rank_addr.h"

namespace sd {

namespace {

using namespace rank;

// features [k, k + 4) of point pt of sequence b, zeros outside (points, features); VEC: every row of
// pred and target starts on a 16-byte boundary and features % 4 == 0
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ pred, const float* __restrict__ target, int64_t b,
                                            int pt, int points, int samples, int64_t features, int64_t k) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pt < points && k < features) {
        const float* p = (pt == 0 ? target : pred) + point_offset(b, pt, samples, features) + k;
        if constexpr (VEC) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (k + 1 < features) v.y = p[1];
            if (k + 2 < features) v.z = p[2];
            if (k + 3 < features) v.w = p[3];
        }
    }
    return v;
}

__device__ __forceinline__ float comp(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

template <bool VEC>
__global__ __launch_bounds__(kDistThreads) void k_rank_dist(const float* __restrict__ pred,
                                                            const float* __restrict__ target, int samples,
                                                            int64_t features, int npairs, float* __restrict__ dist) {
    __shared__ float4 As[2][kKQ * kLd];
    __shared__ float4 Bs[2][kKQ * kLd];
    const int points = samples + 1;
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / npairs;
    int ti, tj;
    pair_tiles((int)((int64_t)blockIdx.x - b * npairs), tiles(points), &ti, &tj);
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int lkq = load_kq(tid);

    float4 pa[kQ], pb[kQ];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            pa[q] = load_quad<VEC>(pred, target, b, i0 + load_row(tid, q), points, samples, features, k0 + 4 * lkq);
#pragma unroll
        for (int q = 0; q < kQ; ++q)
            pb[q] = load_quad<VEC>(pred, target, b, j0 + load_row(tid, q), points, samples, features, k0 + 4 * lkq);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            As[buf][a_slot(lkq, load_row(tid, q))] = pa[q];
            Bs[buf][b_slot(lkq, load_row(tid, q))] = pb[q];
        }
    };

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    const int64_t nchunks = (features + kKC - 1) / kKC;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int64_t c = 0; c < nchunks; ++c) {
        const int buf = (int)(c & 1);
        const bool more = c + 1 < nchunks;
        if (more) gload((c + 1) * kKC);  // in flight during this chunk's arithmetic
        float t[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t[i][j] = 0.f;
        // k quads that hold a feature; the ones past the end would add fma(0, 0, t) = t
        const int nkq = chunk_quads(features, c);
#pragma unroll 2
        for (int kq = 0; kq < nkq; ++kq) {
            float4 a[4], bb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[buf][a_slot(kq, out_row(tid, i))];
#pragma unroll
            for (int j = 0; j < 4; ++j) bb[j] = Bs[buf][b_slot(kq, out_col(tid, j))];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = comp(a[i], kk) - comp(bb[j], kk);
                        t[i][j] = fmaf(d, d, t[i][j]);
                    }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + t[i][j];
        // the other buffer was last read in the previous iteration, which every thread left through the
        // barrier below
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = i0 + out_row(tid, i), gj = j0 + out_col(tid, j);
            if (!owns(ti, tj, gi, gj, points)) continue;
            const float v = sqrtf(acc[i][j]);
            dist[dist_offset(b, points, gi, gj)] = v;
            if (gi != gj) dist[dist_offset(b, points, gj, gi)] = v;
        }
}

// arg-max (MAX) or arg-min of the workgroup's candidates (v, i); every thread returns the winner's index
// and, through *best, its value.  Two barriers: the caller may call again at once.
template <bool MAX>
__device__ __forceinline__ int group_best(float v, int i, float* wv, int* wi, float* best) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        meet<MAX>(&v, &i, ov, oi);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wv[threadIdx.x / kWave] = v;
        wi[threadIdx.x / kWave] = i;
    }
    __syncthreads();
    block_best<MAX>(wv, wi, kThreads / kWave, &v, &i);
    __syncthreads();
    *best = v;
    return i;
}

__global__ __launch_bounds__(kThreads) void k_rank_select(const float* __restrict__ dist, int points, int n_choose,
                                                          int from_closest, int64_t* __restrict__ idx_out,
                                                          float* __restrict__ score_out,
                                                          int64_t* __restrict__ closest_out,
                                                          float* __restrict__ dist_out) {
    __shared__ float wv[kThreads / kWave];
    __shared__ int wi[kThreads / kWave];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const float* D = dist + dist_offset(b, points, 0, 0);
    bool live = tid >= 1 && tid < points;  // thread i is candidate point i

    int anchor = 0;  // the matrix row that serves as P_0
    float best;
    if (from_closest) {
        anchor = group_best<false>(live ? D[tid] : 0.f, live ? tid : -1, wv, wi, &best);
        if (tid == 0 && closest_out) closest_out[b] = anchor - 1;
    }
    float m = live ? D[(int64_t)anchor * points + tid] : 0.f;
    for (int k = 0; k < n_choose; ++k) {
        const int c = group_best<true>(m, live ? tid : -1, wv, wi, &best);
        if (tid == 0) {
            idx_out[b * n_choose + k] = c - 1;
            if (score_out) score_out[b * n_choose + k] = best;
        }
        if (tid == c) live = false;
        if (live) m = min_nan(m, D[(int64_t)c * points + tid]);
    }
    if (dist_out) {  // the matrix of [anchor; samples]: row and column 0 are the anchor's
        float* O = dist_out + dist_offset(b, points, 0, 0);
        for (int e = tid; e < points * points; e += kThreads) {
            const int i = e / points, j = e - i * points;
            O[e] = D[(int64_t)anchored(i, anchor) * points + anchored(j, anchor)];
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int rank_check(int64_t nseq, int32_t samples, int64_t features, int32_t n_choose, int32_t from_closest) {
    if (nseq < 0) return set_error(SD_E_INVALID, "diverse_rank: nseq must be >= 0");
    if (samples < 1 || samples > kMaxPoints - 1)
        return set_error(SD_E_INVALID, "diverse_rank: samples must be in 1.." + std::to_string(kMaxPoints - 1));
    if (features < 1) return set_error(SD_E_INVALID, "diverse_rank: features must be >= 1");
    if (n_choose < 1 || n_choose > samples) return set_error(SD_E_INVALID, "diverse_rank: n_choose must be in 1..samples");
    if (from_closest != 0 && from_closest != 1) return set_error(SD_E_INVALID, "diverse_rank: from_closest must be 0 or 1");
    if (nseq > INT32_MAX / tile_pairs(samples + 1))
        return set_error(SD_E_INVALID, "diverse_rank: nseq exceeds 2^31 - 1 tile pairs");
    return SD_OK;
}

}  // namespace

}  // namespace sd

extern "C" {

size_t sd_diverse_rank_workspace_bytes(int64_t nseq, int32_t samples) {
    using namespace sd;
    if (nseq < 0 || samples < 1 || samples > rank::kMaxPoints - 1) return 0;
    return (size_t)nseq * (size_t)(samples + 1) * (size_t)(samples + 1) * sizeof(float);
}

int sd_diverse_rank(const float* pred, const float* target, int64_t nseq, int32_t samples, int64_t features,
                    int32_t n_choose, int32_t from_closest, int64_t* idx_out, float* score_out, int64_t* closest_out,
                    float* dist_out, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sd;
    if (const int rc = rank_check(nseq, samples, features, n_choose, from_closest)) return rc;
    if (nseq == 0) return SD_OK;
    if (!pred) return set_error(SD_E_INVALID, "diverse_rank: pred is null");
    if (!target) return set_error(SD_E_INVALID, "diverse_rank: target is null");
    if (!idx_out) return set_error(SD_E_INVALID, "diverse_rank: idx_out is null");
    if (closest_out && !from_closest) return set_error(SD_E_INVALID, "diverse_rank: closest_out given with from_closest = 0");
    if (!workspace) return set_error(SD_E_INVALID, "diverse_rank: workspace is null");
    if (workspace_bytes < sd_diverse_rank_workspace_bytes(nseq, samples))
        return set_error(SD_E_INVALID, "diverse_rank: workspace_bytes is smaller than sd_diverse_rank_workspace_bytes");
    hipStream_t s = (hipStream_t)stream;
    const int points = samples + 1, npairs = rank::tile_pairs(points);
    float* dist = (float*)workspace;
    const bool vec = features % 4 == 0 && aligned16(pred) && aligned16(target);
    hipLaunchKernelGGL(vec ? k_rank_dist<true> : k_rank_dist<false>, dim3((unsigned)(nseq * npairs)), dim3(kDistThreads), 0, s,
                       pred, target, (int)samples, features, npairs, dist);
    SD_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rank_select, dim3((unsigned)nseq), dim3(rank::kThreads), 0, s, (const float*)dist, points,
                       (int)n_choose, (int)from_closest, idx_out, score_out, closest_out, dist_out);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // extern "C"
