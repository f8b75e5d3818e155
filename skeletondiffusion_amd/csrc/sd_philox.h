// The device random stream every kernel here draws from (the sampler's noise in sd_kernels.hip, the
// data augmentation in sd_motion_batch.hip): counter-based Philox4x32-10 (Salmon et al. SC'11) +
// Box-Muller.
// ctr = (quad q within the row, step, row lo, row hi), key = (seed lo, seed hi);
// u = ((x >> 8) + 0.5) * 2^-24; z = sqrt(-2 ln u0) * (cos, sin)(2 pi u1), (u2, u3) likewise.
// The same stream as oracle/skeldiff_oracle.py:philox_normal: the Philox words bit for bit, the
// normals within the hardware transcendentals' error (box_muller).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_device.h"

namespace sd {

__device__ __forceinline__ uint4 philox(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 32 x 32 -> 64-bit product per word (v_mad_u64_u32) instead of a mul_hi + mul_lo pair
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// Box-Muller on the exact uniforms u = (2 m + 1) 2^-25, m = x >> 8 (the oracle's, in float64).  In
// float32 u = n 2^-25 (n = 2 m + 1) is exact below 1/2 only (above, the spacing is 2^-24), and
// next to u0 = 1, where rad is small, ln u0 needs relative accuracy (float32 u0 and the hardware
// v_log_f32 each moved z by up to ~5e-5 there).  Two forms, both evaluated and one selected (no
// lane-divergent branch): u0 > 1 - 2^-6: ln u0 = log1p(x) with x = -(2^25 - n) 2^-25 exact, by its
// degree-5 Taylor polynomial (truncation < x^5 / 6, 1.4e-10 relative); otherwise v_log_f32 of the
// float32 u0 (relative rounding 2^-25, i.e. <= 3e-8 absolute in ln u0 where rad >= 0.17).  ~15 VALU
// instead of a float64 log (~60 FP64 instructions) or ocml's log1pf (~100).  (cos, sin)(2 pi u1) by an exact
// quadrant reduction in integers: q = round(n / 2^23), theta = (n - q 2^23) 2 pi 2^-25 in
// [-pi/4, pi/4], degree-9 / -8 Taylor polynomials (truncation < 3e-9) and the quadrant's rotation
// (~20 VALU per pair, not sincospif's general range reduction).  Within a few ulp of the exact
// transform; tests/test_gpu_parity.py holds 4.9 M normals to 2e-5 of the oracle.
__device__ __forceinline__ floatx2 box_muller(uint32_t a, uint32_t b) {
    const uint32_t n0 = 2u * (a >> 8) + 1u;
    const uint32_t r0 = (1u << 25) - n0;                                   // 1 - u0 = r0 2^-25
    const float lg = __builtin_amdgcn_logf((float)n0 * 2.98023223876953125e-8f) * 0.693147180559945309f;
    const float x = -(float)r0 * 2.98023223876953125e-8f;                  // u0 - 1, exact (r0 < 2^19)
    float pl = fmaf(x, 0.2f, -0.25f);                                      // log1p: x - x^2/2 + ... + x^5/5
    pl = fmaf(x, pl, 0.333333343f);
    pl = fmaf(x, pl, -0.5f);
    pl = fmaf(x, pl, 1.0f);
    const float lnu = r0 < (1u << 19) ? x * pl : lg;
    const float rad = __builtin_amdgcn_sqrtf(-2.0f * lnu);
    const int n = (int)(2u * (b >> 8) + 1u);      // u1 = n 2^-25
    const int q = (n + (1 << 22)) >> 23;          // nearest quarter turn, 0 .. 4
    const float th = (float)(n - (q << 23)) * 1.87253514863e-7f;  // 2 pi 2^-25
    const float t2 = th * th;
    float sn = fmaf(t2, 2.7557319e-6f, -1.9841270e-4f);      // 1/9!, -1/7!
    sn = fmaf(t2, sn, 8.3333333e-3f);
    sn = fmaf(t2, sn, -1.6666667e-1f);
    sn = fmaf(t2 * th, sn, th);
    float cs = fmaf(t2, 2.4801587e-5f, -1.3888889e-3f);      // 1/8!, -1/6!
    cs = fmaf(t2, cs, 4.1666667e-2f);
    cs = fmaf(t2, cs, -0.5f);
    cs = fmaf(t2, cs, 1.0f);
    const int qi = q & 3;
    const float c2 = (qi & 1) ? sn : cs, s2 = (qi & 1) ? cs : sn;  // quarter turns: (c, s) -> (-s, c)
    const float cv = (qi == 1 || qi == 2) ? -c2 : c2;
    const float sv = (qi >= 2) ? -s2 : s2;
    return floatx2{rad * cv, rad * sv};
}

__device__ __forceinline__ uint4 philox_at(uint64_t seed, uint64_t row, int step, uint32_t quad) {
    return philox(make_uint4(quad, (uint32_t)step, (uint32_t)row, (uint32_t)(row >> 32)),
                  (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace sd
