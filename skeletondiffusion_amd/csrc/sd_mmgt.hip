// Multimodal ground truth on the device: the reference's get_multimodal_gt
// (src/data/loaders/base/math_utils.py:59-110) measures, for every pair of segments, the L2 distance between
// the last observed poses with torch.cdist(compute_mode='donot_use_mm_for_euclid_dist'), and the APD of a
// segment's multimodal ground truths (src/metrics/multimodal.py:15-35 applied to the set) needs the same
// distance between futures.  Here:
//   k_cdist      dist[i, j] = sqrt(sum_k (x1[i, k] - x2[j, k])^2) from differences, never from
//                |a|^2 + |b|^2 - 2 a.b; one 256-thread workgroup per 128 x 64 tile of dist, 8 x 4 outputs per
//                thread, the feature axis streamed through LDS in chunks of 32 with the next chunk's global
//                loads in flight; there is no matrix-instruction form of (a - b)^2, so this is a VALU kernel;
//   k_set_mean   per set of a CSR adjacency the mean of dist over the set's pairs a < b.
//
// Summation order of k_cdist (the one fixed blocked order; the contract of sd_cdist rests on it).  The
// features are cut into chunks of kKC = 32 from feature 0 on, the last one padded with zeros.  Within a
// chunk: t = 0, then t = fma(d_k, d_k, t) for k ascending, d_k = x1[i, k] - x2[j, k] (one rounding per
// step).  Across chunks: acc = 0, then acc = acc + t in chunk order.  Last, the correctly rounded sqrt.
// Nothing else enters: not m, n, the tile, the thread, or how the operands were loaded.  (a - b)^2 and
// (b - a)^2 are the same float, so swapping the operands gives the same bits; fma(0, 0, t) = t and
// acc + 0 = acc exactly, so the zero padding of rows and features is invisible.  The longest chain of
// roundings is kKC inside a chunk plus ceil(features / kKC) across chunks.
//
// LDS layout.  A chunk of a row tile is kept as float4 = four consecutive features of one row, slot
// [k quad][row], so the global rows go to LDS with 16-byte writes and no transpose, and the inner loop
// reads 16 bytes per operand row and k quad.  Thread (tx, ty) owns rows ty + 16 i (i < 8) and columns
// 4 tx + j (j < 4); x2's rows are stored at slot (col & 3) * 16 + (col >> 2), so that for fixed i or j the
// lanes of a wave read consecutive slots (no bank conflict) while a thread's four columns stay adjacent in
// dist for a 16-byte store.  The k-quad stride is padded by two slots: the eight k quads of a row, written
// by eight neighbouring lanes, fall on different banks.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"

namespace sd {

namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128, kTN = 64;  // rows of x1 / of x2 per tile
constexpr int kKC = 32;             // features per chunk (the summation order above)
constexpr int kKQ = kKC / 4;        // k quads per chunk
constexpr int kLdA = kTM + 2, kLdB = kTN + 2;  // float4 slots per k quad
constexpr int kQA = kTM * kKQ / kThreads, kQB = kTN * kKQ / kThreads;  // quads a thread loads per chunk: 4, 2

// features [k, k + 4) of row `row`, zeros outside (rows, features); VEC: every row starts on a 16-byte
// boundary and features % 4 == 0, so a quad is whole and aligned
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ x, int64_t rows, int64_t features, int64_t row,
                                            int64_t k) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows && k < features) {
        const float* p = x + row * features + k;
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

// VIN: both operands take 16-byte loads; VOUT: dist takes 16-byte stores (the same arithmetic either way)
template <bool VIN, bool VOUT>
__global__ __launch_bounds__(kThreads) void k_cdist(const float* __restrict__ x1, int64_t m,
                                                    const float* __restrict__ x2, int64_t n, int64_t features,
                                                    float* __restrict__ dist, int64_t tiles_n) {
    __shared__ float4 As[2][kKQ * kLdA];
    __shared__ float4 Bs[2][kKQ * kLdB];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t bm = (int64_t)blockIdx.x / tiles_n, bn = (int64_t)blockIdx.x - bm * tiles_n;
    const int64_t i0 = bm * kTM, j0 = bn * kTN;
    const int lrow = tid >> 3, lkq = tid & 7;  // loader role: quad q of the thread is row lrow + 32 q, k quad lkq

    float4 pa[kQA], pb[kQB];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < kQA; ++q) pa[q] = load_quad<VIN>(x1, m, features, i0 + lrow + 32 * q, k0 + 4 * lkq);
#pragma unroll
        for (int q = 0; q < kQB; ++q) pb[q] = load_quad<VIN>(x2, n, features, j0 + lrow + 32 * q, k0 + 4 * lkq);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < kQA; ++q) As[buf][lkq * kLdA + lrow + 32 * q] = pa[q];
#pragma unroll
        for (int q = 0; q < kQB; ++q) {
            const int col = lrow + 32 * q;
            Bs[buf][lkq * kLdB + (col & 3) * 16 + (col >> 2)] = pb[q];
        }
    };

    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
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
        float t[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) t[i][j] = 0.f;
        // k quads that hold a feature; the ones past the end are all zeros and would add fma(0, 0, t) = t.
        // (Not unrolled: one k quad's operands are 48 registers, and three workgroups share a CU.)
        const int nkq = (int)min((int64_t)kKQ, (features - c * kKC + 3) / 4);
#pragma unroll 1
        for (int kq = 0; kq < nkq; ++kq) {
            float4 a[8], b[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = As[buf][kq * kLdA + ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[buf][kq * kLdB + 16 * j + tx];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = comp(a[i], kk) - comp(b[j], kk);
                        t[i][j] = fmaf(d, d, t[i][j]);
                    }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + t[i][j];
        // the other buffer was last read in the previous iteration, which every thread left through the
        // barrier below
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }

    const int64_t c0 = j0 + 4 * tx;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t r = i0 + ty + 16 * i;
        if (r >= m || c0 >= n) continue;
        float* o = dist + r * n + c0;
        const float4 v = make_float4(sqrtf(acc[i][0]), sqrtf(acc[i][1]), sqrtf(acc[i][2]), sqrtf(acc[i][3]));
        if constexpr (VOUT) {  // n % 4 == 0: a quad that starts inside a row ends inside it
            *reinterpret_cast<float4*>(o) = v;
        } else {
            o[0] = v.x;
            if (c0 + 1 < n) o[1] = v.y;
            if (c0 + 2 < n) o[2] = v.z;
            if (c0 + 3 < n) o[3] = v.w;
        }
    }
}

// One workgroup per set s: members col[row_ptr[s] .. row_ptr[s + 1]).  Wave w takes the first members
// a = w, w + 4, ...; its lanes the partners b = a + 1 + lane, + 64, ...; every lane adds its terms in that
// order in float64; the 64 lanes meet in an xor butterfly and the 4 waves as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(kThreads) void k_set_mean(const float* __restrict__ dist, int64_t n,
                                                       const int64_t* __restrict__ row_ptr,
                                                       const int64_t* __restrict__ col, int64_t nsets,
                                                       float* __restrict__ out) {
    __shared__ double wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t s = blockIdx.x; s < nsets; s += gridDim.x) {  // uniform over the workgroup
        const int64_t beg = row_ptr[s], cnt = row_ptr[s + 1] - beg;
        if (cnt <= 1) {  // multimodal.py:19-20 for one member; the mean of no pairs of no members is NaN
            if (tid == 0) out[s] = cnt == 1 ? 0.f : __builtin_nanf("");
            continue;
        }
        double acc = 0.0;
        for (int64_t a = wave; a < cnt - 1; a += 4) {
            const float* row = dist + col[beg + a] * n;
            for (int64_t b = a + 1 + lane; b < cnt; b += 64) acc += (double)row[col[beg + b]];
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            const double pairs = 0.5 * (double)cnt * (double)(cnt - 1);
            out[s] = (float)(((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) / pairs);
        }
        __syncthreads();
    }
}

int hip_fail(const char* what, hipError_t e) { return set_error(SD_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

}  // namespace sd

extern "C" {

int sd_cdist(const float* x1, int64_t m, const float* x2, int64_t n, int64_t features, float* dist, void* stream) {
    using namespace sd;
    if (m < 0) return set_error(SD_E_INVALID, "cdist: m must be >= 0");
    if (n < 0) return set_error(SD_E_INVALID, "cdist: n must be >= 0");
    if (features < 1) return set_error(SD_E_INVALID, "cdist: features must be >= 1");
    if (m == 0 || n == 0) return SD_OK;
    if (!x1) return set_error(SD_E_INVALID, "cdist: x1 is null");
    if (!x2) return set_error(SD_E_INVALID, "cdist: x2 is null");
    if (!dist) return set_error(SD_E_INVALID, "cdist: dist is null");
    const int64_t tiles_m = (m + kTM - 1) / kTM, tiles_n = (n + kTN - 1) / kTN;
    if (tiles_m > INT32_MAX / tiles_n) return set_error(SD_E_INVALID, "cdist: m * n exceeds 2^31 - 1 tiles of 128 x 64");
    const bool vin = features % 4 == 0 && aligned16(x1) && aligned16(x2), vout = n % 4 == 0 && aligned16(dist);
    const auto kernel = vin ? (vout ? k_cdist<true, true> : k_cdist<true, false>)
                            : (vout ? k_cdist<false, true> : k_cdist<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(kThreads), 0, (hipStream_t)stream, x1, m, x2, n,
                       features, dist, tiles_n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_cdist", e);
}

int sd_set_mean_distance(const float* dist, int64_t n, const int64_t* row_ptr, const int64_t* col, int64_t nsets,
                         float* out, void* stream) {
    using namespace sd;
    if (n < 0) return set_error(SD_E_INVALID, "set_mean_distance: n must be >= 0");
    if (nsets < 0) return set_error(SD_E_INVALID, "set_mean_distance: nsets must be >= 0");
    if (nsets == 0) return SD_OK;
    if (!row_ptr) return set_error(SD_E_INVALID, "set_mean_distance: row_ptr is null");
    if (!out) return set_error(SD_E_INVALID, "set_mean_distance: out is null");
    if (n > 0 && !dist) return set_error(SD_E_INVALID, "set_mean_distance: dist is null");
    if (n > 0 && !col) return set_error(SD_E_INVALID, "set_mean_distance: col is null");
    const unsigned grid = (unsigned)(nsets < ((int64_t)1 << 20) ? nsets : ((int64_t)1 << 20));
    hipLaunchKernelGGL(k_set_mean, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, dist, n, row_ptr, col, nsets, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_set_mean", e);
}

}  // extern "C"
