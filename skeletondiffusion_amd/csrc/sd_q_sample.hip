// The forward process q(x_t | x_0) for k noisy copies of every training sequence, one
// kernel for what p_losses does with repeat_interleave, randn and q_sample:
//   x_t[r, i, d] = sqrt_ac[t_s] x0[s, i, d] + sum_j M[t_s, i, j] eps[r, j, d]     (M = Umm_sqrt_Lambda_bar_t)
//   x_t[r, i, d] = sqrt_ac[t_s] x0[s, i, d] + sqrt_1mac[t_s] eps[r, i, d]          (isotropic)
// for row r = copy `copy` of sequence s; eps drawn from the sampler's Philox stream keyed by the row's
// place in the full launch, or read from a supplied tensor.  With `sel` only the copy sel[s] of each
// sequence is produced, bit for bit the row the full launch writes: the selected pass of the best-of-k
// step regenerates its input instead of keeping nseq k rows.
//   k_q_sample_groups   one workgroup per output row.  Pass 1: each thread draws (or reads) quads of the
//                       row's J D normals, writes them to noise_out when asked, and either finishes the
//                       isotropic row there or leaves them in LDS.  Pass 2 (M): one thread per (joint i,
//                       feature quad) sums over the J joints from LDS and row i of M[t].
// Every offset, LDS index, loop bound and sum comes from sd_q_sample_addr.h; tests/host/q_sample_emulation.cpp
// walks the same functions.  All global accesses of rows are 16-byte vectors (D % 4 == 0, bases checked).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_philox.h"
#include "sd_q_sample_addr.h"

namespace sd {

namespace {

using namespace qsample;

struct QSampleArgs {
    const float* x0; const int64_t* t; const float* sqrt_ac; const float* M; const float* sqrt_1mac;
    int T, k, J, D;
    const int64_t* sel; const float* noise_in;
    uint64_t seed; int step; int64_t row0;
    float* x_t; float* noise_out;
};

__global__ __launch_bounds__(kThreads) void k_q_sample_groups(QSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_eps[];  // [J][D] the row's noise (M form only)
    const int tid = threadIdx.x;
    const int J = a.J, D = a.D, Q = quads(J, D);
    const int64_t o = blockIdx.x;
    const bool has_sel = a.sel != nullptr;
    const RowMap rm = row_map(o, a.k, has_sel, has_sel ? a.sel[o] : 0, a.row0);
    const int t = clamp_t(a.t[rm.seq], a.T);
    const float ca = a.sqrt_ac[t];
    const float cb = a.M ? 0.f : a.sqrt_1mac[t];
    for (int q = tid; q < Q; q += kThreads) {
        const int e = quad_elem(q);
        floatx4 v;
        if (a.noise_in) {
            v = *reinterpret_cast<const floatx4*>(a.noise_in + row_elem(rm.noise_row, J, D, e));
        } else {
            const uint4 x = philox_at(a.seed, rm.philox_row, a.step, (uint32_t)q);
            const floatx2 z0 = box_muller(x.x, x.y), z1 = box_muller(x.z, x.w);
            v = floatx4{z0.x, z0.y, z1.x, z1.y};
        }
        if (a.noise_out) *reinterpret_cast<floatx4*>(a.noise_out + row_elem(o, J, D, e)) = v;
        if (a.M) {
            *reinterpret_cast<floatx4*>(s_eps + e) = v;
        } else {
            const floatx4 xs = *reinterpret_cast<const floatx4*>(a.x0 + row_elem(rm.seq, J, D, e));
            const float x0q[4] = {xs.x, xs.y, xs.z, xs.w}, eq[4] = {v.x, v.y, v.z, v.w};
            float r[4];
            iso_quad(ca, x0q, cb, eq, r);
            *reinterpret_cast<floatx4*>(a.x_t + row_elem(o, J, D, e)) = floatx4{r[0], r[1], r[2], r[3]};
        }
    }
    if (!a.M) return;  // workgroup-uniform
    __syncthreads();
    for (int q = tid; q < Q; q += kThreads) {
        const int i = item_joint(q, D), d0 = item_d0(q, D), e = i * D + d0;
        const floatx4 xs = *reinterpret_cast<const floatx4*>(a.x0 + row_elem(rm.seq, J, D, e));
        const float x0q[4] = {xs.x, xs.y, xs.z, xs.w};
        float r[4];
        mix_quad(ca, x0q, a.M + m_row(t, J, i), s_eps, J, D, d0, r);
        *reinterpret_cast<floatx4*>(a.x_t + row_elem(o, J, D, e)) = floatx4{r[0], r[1], r[2], r[3]};
    }
}

int bad(const char* what) { return set_error(SD_E_INVALID, std::string("q_sample_groups: ") + what); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

}  // namespace sd

extern "C" {

int sd_q_sample_groups(const float* x0, const int64_t* t, const float* sqrt_alphas_cumprod, const float* M,
                       const float* sqrt_one_minus_alphas_cumprod, int32_t T, int64_t nseq, int32_t k, int32_t J,
                       int32_t D, const int64_t* sel, const float* noise_in, uint64_t seed, int64_t step, int64_t row0,
                       float* x_t, float* noise_out, void* stream) {
    using namespace sd;
    using namespace sd::qsample;
    if (nseq < 0) return bad("nseq must be >= 0");
    if (k < 1) return bad("k must be >= 1");
    if (J < 1 || J > kMaxJoints) return bad("J must be in [1, 64]");
    if (D < kMinDim || D > kMaxDim || D % 4 != 0) return bad("D must be a multiple of 4 in [4, 256]");
    if (T < 1) return bad("T must be >= 1");
    if (step < 0 || step > INT32_MAX) return bad("step must be in [0, 2^31)");
    if (row0 < 0) return bad("row0 must be >= 0");
    if ((M == nullptr) == (sqrt_one_minus_alphas_cumprod == nullptr))
        return bad("exactly one of M and sqrt_one_minus_alphas_cumprod must be given");
    if (nseq == 0) return SD_OK;
    if (!x0) return bad("x0 is null");
    if (!t) return bad("t is null");
    if (!sqrt_alphas_cumprod) return bad("sqrt_alphas_cumprod is null");
    if (!x_t) return bad("x_t is null");
    if (!aligned16(x0)) return bad("x0 must be 16-byte aligned");
    if (!aligned16(x_t)) return bad("x_t must be 16-byte aligned");
    if (!aligned16(noise_in)) return bad("noise_in must be 16-byte aligned");
    if (!aligned16(noise_out)) return bad("noise_out must be 16-byte aligned");
    if (nseq > INT32_MAX / k) return bad("nseq times k exceeds 2^31 - 1 rows");
    const int64_t rows = out_rows(nseq, k, sel != nullptr);
    QSampleArgs a;
    a.x0 = x0; a.t = t; a.sqrt_ac = sqrt_alphas_cumprod; a.M = M; a.sqrt_1mac = sqrt_one_minus_alphas_cumprod;
    a.T = T; a.k = k; a.J = J; a.D = D; a.sel = sel; a.noise_in = noise_in; a.seed = seed; a.step = (int)step;
    a.row0 = row0; a.x_t = x_t; a.noise_out = noise_out;
    const size_t lds = lds_floats(J, D, M != nullptr) * sizeof(float);  // <= 64 KiB
    hipLaunchKernelGGL(k_q_sample_groups, dim3((unsigned)rows), dim3(kThreads), lds, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SD_OK : set_error(SD_E_HIP, std::string("q_sample_groups: ") + hipGetErrorString(e));
}

}  // extern "C"
