// Fused optimizer step for gfx950: the gradient norm and clip coefficient of
// clip_grad_norm_, the Adam / AdamW update and the EMA update, each over ALL tensors of a model in
// one launch per kBatch tensors (reference src/core/trainer.py:33, :93-95, :153, :159, :267-275).
//
// Every kernel is multi-tensor: a launch carries an OptBatch (sd_optim_table.h) in its kernel
// arguments, the tensors' pointers and scalars plus the compact chunk table, and a workgroup
// strides over the launch's chunks (grid capped at kMaxGrid, the memory-bound idiom).  A chunk is
// kChunk consecutive elements of one tensor: a 16-byte body where every array of the tensor is
// 16-byte aligned, a scalar tail for the rest (numel % 4 != 0, a short last chunk, odd alignment).
// No float atomics: the norm's per-chunk partial sums (float64) are reduced by one workgroup in a
// fixed order, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_optim_math.h"
#include "sd_optim_table.h"

namespace sd {
namespace optim {
namespace {

constexpr int kMaxGrid = 2048;  // 256 CUs x 8 workgroups of 256 threads
constexpr int kWaves = kThreads / 64;

struct ChunkRef {
    int t;
    int64_t off;
    int count;
};
__device__ inline ChunkRef chunk_ref(const OptBatch& b, int64_t c) {
    ChunkRef r;
    r.t = tensor_of(b.first, b.n, c);
    r.off = (c - b.first[r.t]) * kChunk;
    r.count = chunk_count(b.t[r.t].numel, r.off);
    return r;
}

// sum over the workgroup in a fixed order (lanes by shuffle, then the waves in order); valid in thread 0
__device__ inline double block_sum(double x, double* sh) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // sh may still be read from the previous chunk
    if (lane == 0) sh[wave] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kWaves; ++w) s += sh[w];
    return s;
}

// partials[chunk_base + c] = sum of g^2 over chunk c, in float64 (a float32 square is exact there)
__global__ __launch_bounds__(kThreads) void k_opt_norm(const OptBatch b, double* __restrict__ partials) {
    __shared__ double sh[kWaves];
    const int64_t nchunks = b.first[b.n];
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const ChunkRef r = chunk_ref(b, c);
        const float* g = b.t[r.t].g + r.off;
        const int body = vec_body(r.count, (uintptr_t)g);
        double acc = 0.0;
        for (int i = threadIdx.x * 4; i < body; i += kThreads * 4) {
            const float4 x = *reinterpret_cast<const float4*>(g + i);
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        }
        for (int i = body + threadIdx.x; i < r.count; i += kThreads) acc += (double)g[i] * (double)g[i];
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partials[b.chunk_base + c] = s;
    }
}

// one workgroup: total_norm = sqrt(sum of the partials), rounded to float32 once, and the coefficient
__global__ __launch_bounds__(kThreads) void k_opt_norm_final(const double* __restrict__ partials, int64_t n, float max_norm,
                                                             float* __restrict__ norm_coef) {
    __shared__ double sh[kWaves];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) acc += partials[i];
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(s);
        norm_coef[0] = total;
        norm_coef[1] = clip_coef(total, max_norm);
    }
}

__global__ __launch_bounds__(kThreads) void k_opt_step(const OptBatch b, const AdamCall<float> call,
                                                       const float* __restrict__ coef_p) {
    const float coef = coef_p ? *coef_p : 1.f;
    const bool ams = call.flags & kAmsgrad, store_g = call.flags & kStoreGrad;
    const int64_t nchunks = b.first[b.n];
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const ChunkRef r = chunk_ref(b, c);
        const OptTensor& T = b.t[r.t];
        float* p = T.p + r.off;
        float* g = T.g + r.off;
        float* m = T.m + r.off;
        float* v = T.v + r.off;
        float* vm = ams ? T.vmax + r.off : nullptr;
        const AdamTensor<float> ts{T.decay, T.step_size, T.bc2_sqrt};
        const int body = vec_body(r.count, (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vm);
#pragma unroll 2
        for (int i = threadIdx.x * 4; i < body; i += kThreads * 4) {
            float4 P = *reinterpret_cast<const float4*>(p + i);
            float4 G = *reinterpret_cast<const float4*>(g + i);
            float4 M = *reinterpret_cast<const float4*>(m + i);
            float4 V = *reinterpret_cast<const float4*>(v + i);
            float4 X = ams ? *reinterpret_cast<const float4*>(vm + i) : float4{0.f, 0.f, 0.f, 0.f};
            adam_update(P.x, G.x, M.x, V.x, X.x, coef, call, ts);
            adam_update(P.y, G.y, M.y, V.y, X.y, coef, call, ts);
            adam_update(P.z, G.z, M.z, V.z, X.z, coef, call, ts);
            adam_update(P.w, G.w, M.w, V.w, X.w, coef, call, ts);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
            if (ams) *reinterpret_cast<float4*>(vm + i) = X;
            if (store_g) *reinterpret_cast<float4*>(g + i) = G;
        }
        for (int i = body + threadIdx.x; i < r.count; i += kThreads) {
            float P = p[i], G = g[i], M = m[i], V = v[i], X = ams ? vm[i] : 0.f;
            adam_update(P, G, M, V, X, coef, call, ts);
            p[i] = P;
            m[i] = M;
            v[i] = V;
            if (ams) vm[i] = X;
            if (store_g) g[i] = G;
        }
    }
}

// avg (OptTensor::m) <- lerp(avg, live parameter (OptTensor::p), w)
__global__ __launch_bounds__(kThreads) void k_opt_ema(const OptBatch b, float w) {
    const int64_t nchunks = b.first[b.n];
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const ChunkRef r = chunk_ref(b, c);
        const float* p = b.t[r.t].p + r.off;
        float* a = b.t[r.t].m + r.off;
        const int body = vec_body(r.count, (uintptr_t)p | (uintptr_t)a);
#pragma unroll 2
        for (int i = threadIdx.x * 4; i < body; i += kThreads * 4) {
            const float4 P = *reinterpret_cast<const float4*>(p + i);
            float4 A = *reinterpret_cast<const float4*>(a + i);
            A.x = lerp2(A.x, P.x, w);
            A.y = lerp2(A.y, P.y, w);
            A.z = lerp2(A.z, P.z, w);
            A.w = lerp2(A.w, P.w, w);
            *reinterpret_cast<float4*>(a + i) = A;
        }
        for (int i = body + threadIdx.x; i < r.count; i += kThreads) a[i] = lerp2(a[i], p[i], w);
    }
}

unsigned grid_of(const OptBatch& b) {
    const int64_t c = b.first[b.n];
    return (unsigned)(c < kMaxGrid ? c : kMaxGrid);
}

}  // namespace
}  // namespace optim
}  // namespace sd

namespace {
int bad(const char* fn, const std::string& what) { return sd::set_error(SD_E_INVALID, std::string(fn) + ": " + what); }
}  // namespace

extern "C" {

size_t sd_optim_workspace_bytes(const int64_t* numel, int32_t n_tensors) {
    if (!numel || n_tensors <= 0) return 0;
    for (int i = 0; i < n_tensors; ++i)
        if (numel[i] < 0) return 0;
    return (size_t)sd::optim::total_chunks(numel, n_tensors) * sizeof(double);
}

int sd_optim_grad_norm(const float* const* grads, const int64_t* numel, int32_t n_tensors, float max_norm,
                       float* norm_coef, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sd::optim;
    const char* fn = "sd_optim_grad_norm";
    if (n_tensors < 0) return bad(fn, "n_tensors < 0");
    if (!(max_norm > 0.f)) return bad(fn, "max_norm must be > 0");
    if (n_tensors == 0) return SD_OK;
    if (!grads) return bad(fn, "grads is null");
    if (!numel) return bad(fn, "numel is null");
    if (!norm_coef) return bad(fn, "norm_coef is null");
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return bad(fn, "numel[" + std::to_string(i) + "] < 0");
        if (numel[i] > 0 && !grads[i]) return bad(fn, "grads[" + std::to_string(i) + "] is null");
    }
    const int64_t chunks = total_chunks(numel, n_tensors);
    if (chunks > 0 && (!workspace || workspace_bytes < (size_t)chunks * sizeof(double)))
        return bad(fn, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double* partials = (double*)workspace;
    const std::vector<OptBatch> batches =
        build_batches(numel, n_tensors, [&](int i, OptTensor* t) { t->g = const_cast<float*>(grads[i]); });
    for (const OptBatch& b : batches) {
        hipLaunchKernelGGL(k_opt_norm, dim3(grid_of(b)), dim3(kThreads), 0, s, b, partials);
        SD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_opt_norm_final, dim3(1), dim3(kThreads), 0, s, partials, chunks, max_norm, norm_coef);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_optim_adam_step(const sd_optim_param* params, int32_t n_tensors, double beta1, double beta2, double eps,
                       int32_t flags, const float* coef, void* stream) {
    using namespace sd::optim;
    const char* fn = "sd_optim_adam_step";
    if (n_tensors < 0) return bad(fn, "n_tensors < 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return bad(fn, "beta1 outside [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return bad(fn, "beta2 outside [0, 1)");
    if (!(eps >= 0.0)) return bad(fn, "eps < 0");
    if (flags & ~(SD_OPTIM_AMSGRAD | SD_OPTIM_DECOUPLED_WD | SD_OPTIM_STORE_GRADS)) return bad(fn, "unknown flags");
    if (n_tensors == 0) return SD_OK;
    if (!params) return bad(fn, "params is null");
    std::vector<int64_t> numel((size_t)n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        const sd_optim_param& q = params[i];
        const std::string at = "params[" + std::to_string(i) + "].";
        if (q.numel < 0) return bad(fn, at + "numel < 0");
        if (!(q.lr >= 0.0)) return bad(fn, at + "lr < 0");
        if (!(q.weight_decay >= 0.0)) return bad(fn, at + "weight_decay < 0");
        if (q.step < 1) return bad(fn, at + "step < 1");
        if (q.numel > 0) {
            if (!q.p) return bad(fn, at + "p is null");
            if (!q.grad) return bad(fn, at + "grad is null");
            if (!q.exp_avg) return bad(fn, at + "exp_avg is null");
            if (!q.exp_avg_sq) return bad(fn, at + "exp_avg_sq is null");
            if ((flags & SD_OPTIM_AMSGRAD) && !q.max_exp_avg_sq) return bad(fn, at + "max_exp_avg_sq is null");
        }
        numel[(size_t)i] = q.numel;
    }
    static_assert(SD_OPTIM_AMSGRAD == kAmsgrad && SD_OPTIM_DECOUPLED_WD == kDecoupled && SD_OPTIM_STORE_GRADS == kStoreGrad,
                  "the header's flags are the kernels'");
    const AdamCall<float> call{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, flags};
    const std::vector<OptBatch> batches = build_batches(numel.data(), n_tensors, [&](int i, OptTensor* t) {
        const sd_optim_param& q = params[i];
        t->p = q.p;
        t->g = q.grad;
        t->m = q.exp_avg;
        t->v = q.exp_avg_sq;
        t->vmax = (flags & SD_OPTIM_AMSGRAD) ? q.max_exp_avg_sq : nullptr;
        // as torch computes them: in double from the step count, rounded to float32 once
        const double bc1 = 1.0 - pow(beta1, (double)q.step), bc2 = 1.0 - pow(beta2, (double)q.step);
        t->decay = (flags & SD_OPTIM_DECOUPLED_WD) ? (float)(1.0 - q.lr * q.weight_decay) : (float)q.weight_decay;
        t->step_size = (float)(q.lr / bc1);
        t->bc2_sqrt = (float)sqrt(bc2);
    });
    hipStream_t s = (hipStream_t)stream;
    for (const OptBatch& b : batches) {
        hipLaunchKernelGGL(k_opt_step, dim3(grid_of(b)), dim3(kThreads), 0, s, b, call, coef);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

int sd_optim_ema_update(float* const* ema, const float* const* params, const int64_t* numel, int32_t n_tensors,
                        float weight, void* stream) {
    using namespace sd::optim;
    const char* fn = "sd_optim_ema_update";
    if (n_tensors < 0) return bad(fn, "n_tensors < 0");
    if (!(weight >= 0.f && weight <= 1.f)) return bad(fn, "weight outside [0, 1]");
    if (n_tensors == 0) return SD_OK;
    if (!ema) return bad(fn, "ema is null");
    if (!params) return bad(fn, "params is null");
    if (!numel) return bad(fn, "numel is null");
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0) return bad(fn, "numel[" + std::to_string(i) + "] < 0");
        if (numel[i] > 0 && !ema[i]) return bad(fn, "ema[" + std::to_string(i) + "] is null");
        if (numel[i] > 0 && !params[i]) return bad(fn, "params[" + std::to_string(i) + "] is null");
    }
    const std::vector<OptBatch> batches = build_batches(numel, n_tensors, [&](int i, OptTensor* t) {
        t->p = const_cast<float*>(params[i]);
        t->m = ema[i];
    });
    hipStream_t s = (hipStream_t)stream;
    for (const OptBatch& b : batches) {
        hipLaunchKernelGGL(k_opt_ema, dim3(grid_of(b)), dim3(kThreads), 0, s, b, weight);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

}  // extern "C"
