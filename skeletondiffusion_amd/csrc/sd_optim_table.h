// Tensor and chunk tables of the fused optimizer step (sd_optim.hip).  Host code with no HIP in it:
// the library builds its launches with it, and tests/host/optim_emulation.cpp includes it to walk
// the same tables under AddressSanitizer.
//
// The tables travel as KERNEL ARGUMENTS, one OptBatch per launch: the runtime copies a launch's
// arguments when the launch is enqueued, so no host staging buffer outlives the call, nothing has
// to be kept alive or fenced between steps, and gradient pointers may change from step to step.
#pragma once
#include <stdint.h>

#include <vector>

#include "sd_optim_math.h"

namespace sd {
namespace optim {

// One tensor of a launch.  The step kernel uses every field; the norm kernel reads g; the EMA
// kernel reads p (the live parameter) and writes m (the average).
struct OptTensor {
    float* p;
    float* g;
    float* m;
    float* v;
    float* vmax;
    int64_t numel;
    float decay, step_size, bc2_sqrt, pad_;
};

// The chunk table in its compact form: chunk c of the launch (0 <= c < first[n]) belongs to tensor
// t = tensor_of(first, n, c) and covers elements [off, off + chunk_count(numel, off)) of it with
// off = (c - first[t]) * kChunk.  chunk_base: this launch's first chunk among all launches of the
// call (where its partial sums go).
struct OptBatch {
    OptTensor t[kBatch];
    int64_t first[kBatch + 1];
    int64_t chunk_base;
    int32_t n;
    int32_t pad_;
};
static_assert(sizeof(OptBatch) <= 3584, "an OptBatch and the other arguments must fit the 4 KiB of kernel arguments");

// chunks of all tensors of a call
inline int64_t total_chunks(const int64_t* numel, int n) {
    int64_t c = 0;
    for (int i = 0; i < n; ++i) c += chunks_of(numel[i]);
    return c;
}

// Splits n tensors into launches of at most kBatch tensors each, in order; tensors of no elements
// are left out, and so is a launch without chunks.  fill(i, &slot) sets the pointers and scalars of
// tensor i; numel is set here.
template <class Fill>
inline std::vector<OptBatch> build_batches(const int64_t* numel, int n, Fill fill) {
    std::vector<OptBatch> out;
    OptBatch b{};
    int64_t base = 0;
    auto flush = [&]() {
        if (b.n > 0) {
            out.push_back(b);
            base += b.first[b.n];
        }
        b = OptBatch{};
        b.chunk_base = base;
    };
    for (int i = 0; i < n; ++i) {
        if (numel[i] <= 0) continue;
        if (b.n == kBatch) flush();
        OptTensor& s = b.t[b.n];
        fill(i, &s);
        s.numel = numel[i];
        b.first[b.n + 1] = b.first[b.n] + chunks_of(numel[i]);
        ++b.n;
    }
    flush();
    return out;
}

}  // namespace optim
}  // namespace sd
