// Element math and chunk arithmetic of the fused optimizer step (sd_optim.hip), in one
// __host__ __device__ header: the kernels include it, and so does the stand-alone host program
// tests/host/optim_emulation.cpp, which walks every chunk with this very index arithmetic and
// compares the float32 update with a restatement in double.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_OPT_HD __host__ __device__ inline
#else
#define SD_OPT_HD inline
#endif

namespace sd {
namespace optim {

// A chunk is what one workgroup handles at a time: kChunk consecutive elements of one tensor (the
// last chunk of a tensor may be shorter).  kChunk is a multiple of 4 * kThreads, so a chunk's first
// element is as aligned as the tensor's.
constexpr int kThreads = 256;
constexpr int kChunk = 16384;
// tensors one launch carries in its kernel arguments (OptBatch, sd_optim_table.h)
constexpr int kBatch = 40;

enum StepFlags : int { kAmsgrad = 1, kDecoupled = 2, kStoreGrad = 4 };

SD_OPT_HD float sqrt_(float x) { return sqrtf(x); }
SD_OPT_HD double sqrt_(double x) { return sqrt(x); }

// ---- chunk arithmetic ------------------------------------------------------------------------
SD_OPT_HD int64_t chunks_of(int64_t numel) { return (numel + kChunk - 1) / kChunk; }

// first[0..n] is the running sum of chunks_of(numel) (first[0] = 0); the tensor that chunk c
// (0 <= c < first[n]) belongs to: the last t with first[t] <= c (tensors of no elements own no chunk)
SD_OPT_HD int tensor_of(const int64_t* first, int n, int64_t c) {
    int lo = 0, hi = n;  // invariant: first[lo] <= c < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (first[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}
// elements of the chunk that starts at element `off` of a tensor of numel elements
SD_OPT_HD int chunk_count(int64_t numel, int64_t off) {
    const int64_t left = numel - off;
    return (int)(left < kChunk ? left : kChunk);
}
// A chunk of `count` elements is split into a 16-byte body [0, body) taken four elements at a time
// and a scalar tail [body, count).  addr_bits: the OR of the byte addresses of the chunk's first
// element in every array the kernel touches; unless all are 16-byte aligned the body is empty.
SD_OPT_HD int vec_body(int count, uintptr_t addr_bits) { return (addr_bits & 15) ? 0 : (count & ~3); }

// ---- element math ----------------------------------------------------------------------------
// clip_grad_norm_ (error_if_nonfinite=False): max_norm / (total_norm + 1e-6) clamped to at most 1;
// the comparison keeps a NaN as torch.clamp does
template <class T>
SD_OPT_HD T clip_coef(T total_norm, T max_norm) {
    const T c = max_norm / (total_norm + T(1e-6));
    return c > T(1) ? T(1) : c;
}

// torch.lerp's two-sided form: exact at w = 0 (a) and w = 1 (b)
template <class T>
SD_OPT_HD T lerp2(T a, T b, T w) {
    const T d = b - a;
    return w < T(0.5) ? a + w * d : b - d * (T(1) - w);
}

// per-call scalars of the step (the host computes 1 - beta in double and rounds once)
template <class T>
struct AdamCall {
    T beta1, beta2, omb1, omb2, eps;
    int flags;
};
// per-tensor scalars: decay = 1 - lr wd (AdamW) or wd (Adam L2), step_size = lr / (1 - beta1^t),
// bc2_sqrt = sqrt(1 - beta2^t)
template <class T>
struct AdamTensor {
    T decay, step_size, bc2_sqrt;
};

// One element of the step.  g comes back clipped (what clip_grad_norm_ leaves in p.grad), before
// any L2 term.  vmax is read and written only with kAmsgrad.
template <class T>
SD_OPT_HD void adam_update(T& p, T& g, T& m, T& v, T& vmax, T coef, const AdamCall<T>& c, const AdamTensor<T>& t) {
    g = g * coef;
    T gg = g;
    if (c.flags & kDecoupled) p = p * t.decay;
    else if (t.decay != T(0)) gg = gg + t.decay * p;
    m = c.beta1 * m + c.omb1 * gg;
    v = c.beta2 * v + c.omb2 * (gg * gg);
    T s = v;
    if (c.flags & kAmsgrad) {
        // torch.maximum: a NaN on either side gives NaN
        vmax = (v != v || v > vmax) ? v : vmax;
        s = vmax;
    }
    const T denom = sqrt_(s) / t.bc2_sqrt + c.eps;
    p = p - t.step_size * (m / denom);
}

}  // namespace optim
}  // namespace sd
