// gfx950 (CDNA4, MI355X) kernels of the reverse-diffusion step other than StaticGraphLinear (whose
// generations and dispatcher are in sd_graph_linear*.hip).
//
//   k_attention       multi-head attention over joints, QK^T and PV on MFMA   attention.py:122-136
//   k_attention_mix   the same with the to_qkv layer's node mixing in front (MANO)
//   k_update*         x0 clamp + C1 x0 + C2 x_t + U (sigma . eps)   nonisotropic.py:196-210,
//                     base.py:314-341, isotropic.py:85-95
//   k_noise_fill      counter-based Philox4x32-10 + Box-Muller normals (replaces randn), the raw
//                     Philox words and the device seed record
//   row copies        k_copy_rows, k_convert_rows (f32 <-> bf16)
//   plan helpers      sinusoidal embedding, small linears (time MLP / FiLM tables), G-hat,
//                     RMSNorm gain folding, sigma table
//
// Layout in HBM: every activation is row-major (rows B, nodes J, features F), F contiguous.
// All arithmetic is fp32; the products on the matrix cores use the exact-f32 MFMA (a k-ordered
// fmaf chain).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_device.h"
#include "sd_internal.h"
#include "sd_philox.h"

namespace sd {

__device__ __forceinline__ floatx2 ld2(const float* p) { return *reinterpret_cast<const floatx2*>(p); }
__device__ __forceinline__ void st2(float* p, floatx2 v) { *reinterpret_cast<floatx2*>(p) = v; }
// a latent pair at element offset `o` of a buffer holding f32 or (bf16 mode) bf16 elements
__device__ __forceinline__ floatx2 ld2x(const float* p, int64_t o, int bf) {
    return bf ? __builtin_convertvector(*reinterpret_cast<const bf16x2*>(reinterpret_cast<const __bf16*>(p) + o), floatx2)
              : *reinterpret_cast<const floatx2*>(p + o);
}
__device__ __forceinline__ void st2x(float* p, int64_t o, int bf, floatx2 v) {
    if (bf) *reinterpret_cast<bf16x2*>(reinterpret_cast<__bf16*>(p) + o) = __builtin_convertvector(v, bf16x2);
    else *reinterpret_cast<floatx2*>(p + o) = v;
}

// =============================================================================================
// Attention over joints.  One wave per (row b, head h).  S^T = K Q^T (scaled q, as
// attention.py:128) on 16x16x4 MFMA tiles, softmax over j in registers + 2 lane swaps, then
// O^T = V^T P^T with the S^T accumulator used directly as the B operand (no LDS round trip).
// J <= 16*JT, padded rows/cols masked.
// =============================================================================================

// DH: the head width at compile time (32, the release model: both 16-wide chunks' loads are
// issued together and the V loads with them, so a wave pays one memory latency), 0 = runtime.
// Where the attention reads q / k / v: the (B, J, 3 hid) qkv rows in HBM (k_attention), or one
// head's mixed q | k | v in the wave's LDS region (k_attention_mix).  c: a column of the head
// (0 .. dh - 1), a multiple of 4 for the 16-B forms.
struct AttnSrcG {
    const float* qb; const float* kb; const float* vb; int64_t rs;
    __device__ __forceinline__ floatx4 q4(int j, int c) const { return ld4(qb + j * rs + c); }
    __device__ __forceinline__ floatx4 k4(int j, int c) const { return ld4(kb + j * rs + c); }
    __device__ __forceinline__ floatx4 v4(int j, int c) const { return ld4(vb + j * rs + c); }
    __device__ __forceinline__ float v(int j, int c) const { return vb[j * rs + c]; }
};
// k_attention_mix's region: node j's 96 columns (q | k | v, 32 each) as 24 16-B pieces, piece q at
// q ^ (j & 7) (within its aligned group of 8, so q, k and v stay in their 32-column parts): the
// 16-B reads of 8 consecutive nodes hit 8 different bank groups at the 384-B row stride
struct AttnSrcL {
    const float* s;
    static __device__ __forceinline__ int at(int j, int c) { return j * 96 + (((c >> 2) ^ (j & 7)) << 2) + (c & 3); }
    __device__ __forceinline__ floatx4 q4(int j, int c) const { return ld4(s + at(j, c)); }
    __device__ __forceinline__ floatx4 k4(int j, int c) const { return ld4(s + at(j, 32 + c)); }
    __device__ __forceinline__ floatx4 v4(int j, int c) const { return ld4(s + at(j, 64 + c)); }
    __device__ __forceinline__ float v(int j, int c) const { return s[at(j, 64 + c)]; }
};

// One wave's attention of (row b, head h) from `src` (k_attention's math; every caller the same bits)
template <int JT, int DH, class Src>
__device__ __forceinline__ void attention_body(const AttnArgs& p, const Src& src, int64_t b, int h, int lane) {
    constexpr int JA = JT;  // node tiles as keys / values (round 5's 48-node tail form: git history)
    const int lr = lane & 15, lg = lane >> 4;
    const int J = p.J, dh = DH ? DH : p.dh, hid = p.heads * dh;

    floatx4 S[JT][JT];
#pragma unroll
    for (int a = 0; a < JT; ++a)
#pragma unroll
        for (int c = 0; c < JT; ++c) S[a][c] = floatx4{0.f, 0.f, 0.f, 0.f};

    // unconditional loads from clamped nodes, padding zeroed after: a masked load beside a zero
    // write of the same registers made the compiler wait vmcnt(0) per tile (one memory latency per
    // 16 nodes).  DH = 32: both 16-wide chunks of K and Q and both of V are issued up front, so a
    // wave pays one memory latency
    constexpr int NCC = DH ? DH / 16 : 1;  // chunks loaded together
    floatx4 vv[DH ? NCC : 1][JT];
    auto load_v = [&](int dc, floatx4* v) {
#pragma unroll
        for (int jt = 0; jt < JA; ++jt)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) v[jt][s4] = src.v(min(jt * 16 + 4 * lg + s4, J - 1), dc + lr);
    };
    auto mask_v = [&](floatx4* v) {
#pragma unroll
        for (int jt = 0; jt < JA; ++jt)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) v[jt][s4] = jt * 16 + 4 * lg + s4 < J ? v[jt][s4] : 0.f;
    };
#pragma unroll
    for (int cc0 = 0; cc0 < dh; cc0 += 16 * NCC) {
        floatx4 ka[NCC][JT], qv[NCC][JT];
#pragma unroll
        for (int u = 0; u < NCC; ++u)
#pragma unroll
            for (int t = 0; t < JT; ++t) {
                const int jc = min(t * 16 + lr, J - 1);
                ka[u][t] = src.k4(jc, cc0 + 16 * u + 4 * lg);
                qv[u][t] = src.q4(jc, cc0 + 16 * u + 4 * lg);
            }
        if constexpr (DH != 0) {
#pragma unroll
            for (int u = 0; u < NCC; ++u) load_v(16 * u, vv[u]);
        }
#pragma unroll
        for (int u = 0; u < NCC; ++u) {
#pragma unroll
            for (int t = 0; t < JT; ++t) {
                const bool ok = t * 16 + lr < J;
                ka[u][t] = ok ? ka[u][t] : floatx4{0.f, 0.f, 0.f, 0.f};
                qv[u][t] = ok ? qv[u][t] * p.scale : floatx4{0.f, 0.f, 0.f, 0.f};
            }
            // component-major over the JT x JT tiles: consecutive MFMAs are independent (tile by
            // tile, each waited for the previous one's result); every tile still accumulates its
            // k steps x, y, z, w in order, so the sums are bit-identical
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int jt = 0; jt < JA; ++jt)
#pragma unroll
                    for (int nt = 0; nt < JT; ++nt) S[jt][nt] = mfma4(ka[u][jt][e], qv[u][nt][e], S[jt][nt]);
        }
    }
    // softmax over j (rows of S^T) for every query column n = nt*16 + lr
#pragma unroll
    for (int nt = 0; nt < JT; ++nt) {
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (jt * 16 + 4 * lg + r < J) m = fmaxf(m, S[jt][nt][r]);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = (jt * 16 + 4 * lg + r < J) ? expf(S[jt][nt][r] - m) : 0.f;
                S[jt][nt][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) S[jt][nt] *= inv;
    }

    // O^T[d][n] = sum_j V[j][d] P^T[j][n]
#pragma unroll
    for (int dc = 0; dc < dh; dc += 16) {
        floatx4* v = vv[DH ? dc / 16 : 0];
        if constexpr (DH == 0) load_v(dc, v);
        mask_v(v);
        // the JT output tiles' chains interleaved (each still sums jt-major, x y z w minor)
        floatx4 o[JT];
#pragma unroll
        for (int nt = 0; nt < JT; ++nt) o[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jt = 0; jt < JA; ++jt)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < JT; ++nt) o[nt] = mfma4(v[jt][e], S[jt][nt][e], o[nt]);
#pragma unroll
        for (int nt = 0; nt < JT; ++nt) {
            const int n = nt * 16 + lr;
            if (n < J) {
                float* ob = p.out + (b * J + n) * hid + h * dh + dc + 4 * lg;
                *reinterpret_cast<floatx4*>(ob) = o[nt];
            }
        }
    }
}


template <int JT, int DH = 0>
__global__ __launch_bounds__(256) void k_attention(const AttnArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= p.B * p.heads) return;
    const int64_t b = pair / p.heads;
    const int h = (int)(pair % p.heads);
    const int J = p.J, dh = DH ? DH : p.dh, hid = p.heads * dh;
    const int64_t rs = 3 * (int64_t)hid;
    const float* base = p.qkv + b * J * rs;
    const AttnSrcG src{base + h * dh, base + hid + h * dh, base + 2 * hid + h * dh, rs};
    attention_body<JT, DH>(p, src, b, h, lane);
}

// k_attention_mix (SD_OPT_ATTENTION 2; 49 <= J <= 52, dh = 32: MANO): the to_qkv layer's node mixing
// (its k_gl5_mixd pass) moved into the attention kernel, so the mixed q / k / v never reach HBM --
// the plan's to_qkv launch writes only its pre-mix Y (GLArgs::skip_mix).  Per wave (row b, head h):
//   1. the head's pre-mix Y (J nodes x 96 columns q | k | v) to the wave's LDS region (AttnSrcL),
//      rows J .. 51 zero (k_gl5_mixd's padding rows);
//   2. out[i][c] = sum_j G-hat[i][j] Y[j][c] on v_mfma_f32_16x16x4_f32 with k_gl5_mixd's operands
//      (A = Y^T: 16 columns x 4 nodes, B = G-hat^T fragments, k steps in j order from a zero
//      accumulator, + 0.f as its epilogue adds the absent residual): the same bits;
//   3. the results to the region (all of this wave's Y reads are behind them: the region is the
//      wave's own, no barrier), then k_attention's padded-form body reads q / k / v from it.
// 4 waves x 52 x 96 floats = 78 KiB per workgroup: 2 workgroups per CU.
constexpr int kAttnMixRows = 52;  // 4 ceil(J / 4) at J <= 52
template <int DH>
__global__ __launch_bounds__(256, 2) void k_attention_mix(const AttnArgs p) {
    static_assert(DH == 32, "the MANO head width");
    constexpr int KS = kAttnMixRows / 4, NPC = (kAttnMixRows * 24 + 63) / 64;
    __shared__ __attribute__((aligned(16))) float s_y[4][kAttnMixRows * 96];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l16 = lane & 15, l4 = lane >> 4;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wv;
    if (pair >= p.B * p.heads) return;
    const int64_t b = pair / p.heads;
    const int h = (int)(pair % p.heads);
    const int J = p.J, hid = p.heads * DH;
    const int64_t rs = 3 * (int64_t)hid;
    float* sy = s_y[wv];
    // 1. piece idx = 24 j + q of the region: node j, part q / 8 (q, k, v), columns 4 (q % 8) ..;
    // unconditional loads from clamped nodes, the padding rows zeroed at the LDS store
    const float* yb = p.qkv + b * J * rs + h * DH;
    floatx4 yv[NPC];
#pragma unroll
    for (int e = 0; e < NPC; ++e) {
        const int idx = min(lane + 64 * e, kAttnMixRows * 24 - 1), j = idx / 24, q = idx % 24;
        yv[e] = ld4(yb + min(j, J - 1) * rs + (q >> 3) * hid + 4 * (q & 7));
    }
    float gb[4][KS];  // G-hat[16 ib + l16][4 s + l4] (k_gl5_mixd's B fragments), 0 outside J x J
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int s = 0; s < KS; ++s) gb[ib][s] = p.G[min(16 * ib + l16, J - 1) * J + min(4 * s + l4, J - 1)];
#pragma unroll
    for (int e = 0; e < NPC; ++e) {
        const int idx = lane + 64 * e, j = idx / 24, q = idx % 24;
        if (idx < kAttnMixRows * 24)
            *reinterpret_cast<floatx4*>(sy + AttnSrcL::at(j, 4 * q)) = j < J ? yv[e] : floatx4{0.f, 0.f, 0.f, 0.f};
    }
    // the clamped G-hat loads zeroed outside J x J once they have landed (a select right behind
    // each load -- or a masked load -- waited for it there)
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float g = gb[ib][s];
            asm volatile("" : "+v"(g));
            gb[ib][s] = (16 * ib + l16 < J && 4 * s + l4 < J) ? g : 0.f;
        }
    // 2. the mixing, 6 column blocks of 16 x 4 node blocks; per accumulator k_gl5_mixd's chain
    floatx4 mo[6][4];
#pragma unroll
    for (int cb = 0; cb < 6; ++cb) {
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) mo[cb][ib] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float a = sy[AttnSrcL::at(4 * s + l4, 16 * cb + l16)];
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) mo[cb][ib] = mfma4(a, gb[ib][s], mo[cb][ib]);
        }
    }
    // 3. lane (l16, l4) holds out[i = 16 ib + l16][16 cb + 4 l4 + r]
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
        const int i = 16 * ib + l16;
        if (i < J) {
#pragma unroll
            for (int cb = 0; cb < 6; ++cb)
                *reinterpret_cast<floatx4*>(sy + AttnSrcL::at(i, 16 * cb + 4 * l4)) = mo[cb][ib] + 0.f;
        }
    }
    attention_body<4, DH>(p, AttnSrcL{sy}, b, h, lane);
}

hipError_t launch_attention(const AttnArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    const int64_t waves = a.B * a.heads;
    const dim3 grid((unsigned)((waves + 3) / 4));
    g_route_bits |= kRouteAttention;
    if (a.G) {  // the to_qkv mixing in this kernel (k_attention_mix)
        if (a.dh != 32 || a.J < 49 || a.J > kAttnMixRows) return hipErrorNotSupported;
        g_route_bits |= kRouteAttnMix;
        hipLaunchKernelGGL((k_attention_mix<32>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.dh == 32) {  // the release head width: every load of a wave issued up front
        if (a.J <= 16) hipLaunchKernelGGL((k_attention<1, 32>), grid, dim3(256), 0, s, a);
        else if (a.J <= 32) hipLaunchKernelGGL((k_attention<2, 32>), grid, dim3(256), 0, s, a);
        else if (a.J <= 48) hipLaunchKernelGGL((k_attention<3, 32>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_attention<4, 32>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.J <= 16) hipLaunchKernelGGL((k_attention<1>), grid, dim3(256), 0, s, a);
    else if (a.J <= 32) hipLaunchKernelGGL((k_attention<2>), grid, dim3(256), 0, s, a);
    else if (a.J <= 48) hipLaunchKernelGGL((k_attention<3>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_attention<4>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

// Counter-based noise: Philox4x32-10 + Box-Muller (philox, u01, box_muller, philox_at) live in sd_philox.h.

// normals e and e+1 (e even) of the row
__device__ __forceinline__ floatx2 noise_pair(uint64_t seed, uint64_t row, int step, uint32_t e) {
    const uint4 x = philox_at(seed, row, step, e >> 2);
    return ((e >> 1) & 1) ? box_muller(x.z, x.w) : box_muller(x.x, x.y);
}

__global__ __launch_bounds__(256) void k_noise_fill(float* out, int64_t rows, int64_t quads,
                                                    uint64_t seed, int64_t row0, int step,
                                                    const uint64_t* rng_dev, int64_t row_shift, int bf) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * quads) return;
    if (rng_dev) {
        seed = rng_dev[0];
        row0 = (int64_t)rng_dev[1];
    }
    row0 += row_shift;
    const int64_t r = g / quads;
    const uint32_t q = (uint32_t)(g % quads);
    const uint4 x = philox_at(seed, (uint64_t)(row0 + r), step, q);
    const floatx2 z0 = box_muller(x.x, x.y), z1 = box_muller(x.z, x.w);
    const floatx4 v = {z0.x, z0.y, z1.x, z1.y};
    if (bf) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(out) + 4 * g) = __builtin_convertvector(v, bf16x4);
    else *reinterpret_cast<floatx4*>(out + 4 * g) = v;
}

hipError_t launch_noise_fill(float* out, int64_t rows, int64_t n_per_row, uint64_t seed,
                             int64_t row0, int step, const uint64_t* rng_dev, hipStream_t s,
                             int64_t row_shift, int out_bf16) {
    const int64_t quads = n_per_row / 4;
    const int64_t n = rows * quads;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_noise_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, rows,
                       quads, seed, row0, step, rng_dev, row_shift, out_bf16);
    return hipGetLastError();
}

__global__ void k_philox_raw(uint32_t* out, int64_t rows, int64_t quads, uint64_t seed,
                             int64_t row0, int step) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * quads) return;
    const uint4 x = philox_at(seed, (uint64_t)(row0 + g / quads), step, (uint32_t)(g % quads));
    reinterpret_cast<uint4*>(out)[g] = x;
}

hipError_t launch_philox_raw(uint32_t* out, int64_t rows, int64_t quads, uint64_t seed,
                             int64_t row0, int step, hipStream_t s) {
    const int64_t n = rows * quads;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_philox_raw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, rows,
                       quads, seed, row0, step);
    return hipGetLastError();
}

__global__ void k_set_rng(uint64_t* rng, uint64_t seed, int64_t row0) {
    if (threadIdx.x == 0) {
        rng[0] = seed;
        rng[1] = (uint64_t)row0;
    }
}

hipError_t launch_set_rng(uint64_t* rng_dev, uint64_t seed, int64_t row0, hipStream_t s) {
    hipLaunchKernelGGL(k_set_rng, dim3(1), dim3(64), 0, s, rng_dev, seed, row0);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_copy_rows(float* dst, int64_t dst_rs, const float* src,
                                                   int64_t src_rs, int64_t rows, int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n4 = n / 4;
    if (g >= rows * n4) return;
    const int64_t r = g / n4, c = g % n4;
    *reinterpret_cast<floatx4*>(dst + r * dst_rs + 4 * c) = ld4(src + r * src_rs + 4 * c);
}

__global__ __launch_bounds__(256) void k_convert_rows(void* dst, int dbf, int64_t dst_rs, const void* src, int sbf,
                                                      int64_t src_rs, int64_t rows, int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n4 = n / 4;
    if (g >= rows * n4) return;
    const int64_t r = g / n4, c = 4 * (g % n4);
    const int64_t so = r * src_rs + c, d0 = r * dst_rs + c;
    const floatx4 v = sbf ? __builtin_convertvector(*reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(src) + so), floatx4)
                          : *reinterpret_cast<const floatx4*>(reinterpret_cast<const float*>(src) + so);
    if (dbf) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(dst) + d0) = __builtin_convertvector(v, bf16x4);
    else *reinterpret_cast<floatx4*>(reinterpret_cast<float*>(dst) + d0) = v;
}

hipError_t launch_convert_rows(void* dst, int dst_bf16, int64_t dst_rs, const void* src, int src_bf16,
                               int64_t src_rs, int64_t rows, int64_t n, hipStream_t s) {
    const int64_t tot = rows * (n / 4);
    if (tot <= 0) return hipSuccess;
    if (n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_convert_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, dst, dst_bf16, dst_rs, src,
                       src_bf16, src_rs, rows, n);
    return hipGetLastError();
}

hipError_t launch_copy_rows(float* dst, int64_t dst_rs, const float* src, int64_t src_rs,
                            int64_t rows, int64_t n, hipStream_t s) {
    const int64_t tot = rows * (n / 4);
    if (tot <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, dst,
                       dst_rs, src, src_rs, rows, n);
    return hipGetLastError();
}

// =============================================================================================
// Reverse-step update.  One thread per (row, feature pair): the J values of x0, x_t, eps of
// its two features stay in registers; C1[t], C2[t], U and sigma_t come from LDS as
// wave-uniform broadcasts.  HBM-bound: 4 * J * D * 4 B per row (x0, x_t, eps in; x_{t-1} out).
// =============================================================================================

// isotropic pred_noise / pred_v (isotropic.py:48-70): x0 = a[t] x_t - b[t] act(model_out), each
// product rounded before the difference, as the reference's two tensor products and subtraction
__device__ __forceinline__ floatx2 start_from_pred(const UpdArgs& p, floatx2 xt, floatx2 m) {
    return floatx2{__fmul_rn(p.xa, xt.x) - __fmul_rn(p.xb, m.x), __fmul_rn(p.xa, xt.y) - __fmul_rn(p.xb, m.y)};
}

template <int JM, bool EXACT>
__global__ __launch_bounds__(256) void k_update(const UpdArgs p) {
    const int J = EXACT ? JM : p.J;
    __shared__ float sC1[JM * JM], sC2[JM * JM], sU[JM * JM], sS[JM];
    if (!p.iso) {
        for (int i = threadIdx.x; i < J * J; i += 256) {
            sC1[i] = p.C1[i];
            sC2[i] = p.C2[i];
            sU[i] = p.U[i];
        }
        for (int i = threadIdx.x; i < J; i += 256) sS[i] = p.sig[i];
    }
    __syncthreads();
    const int D = p.D;
    const int DP = D >> 1;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = g / DP;
    if (row >= p.B) return;
    const int d = 2 * (int)(g % DP);
    const int64_t rb = row * (int64_t)J * D;

    uint64_t seed = p.seed;
    int64_t row0 = p.row0;
    if (p.noise_mode == 2 && p.rng_dev) {
        seed = p.rng_dev[0];
        row0 = (int64_t)p.rng_dev[1];
    }
    row0 += p.row_shift;

    floatx2 x0v[JM], xtv[JM], ev[JM];
#pragma unroll
    for (int j = 0; j < JM; ++j) {
        if (!EXACT && j >= J) continue;
        floatx2 a = ld2x(p.x0, rb + j * D + d, p.x0_bf16);
        if (p.act == 1) {
            a.x = tanhf(a.x);
            a.y = tanhf(a.y);
        }
        xtv[j] = ld2x(p.xt, rb + j * D + d, p.xt_bf16);
        if (p.obj) a = start_from_pred(p, xtv[j], a);
        x0v[j] = p.clip ? floatx2{fminf(fmaxf(a.x, -1.f), 1.f), fminf(fmaxf(a.y, -1.f), 1.f)} : a;
        if (p.noise_mode == 1)
            ev[j] = ld2(p.eps + row * p.eps_rs + j * D + d);
        else if (p.noise_mode == 2)
            ev[j] = noise_pair(seed, (uint64_t)(row0 + row), p.step, (uint32_t)(j * D + d));
        else
            ev[j] = floatx2{0.f, 0.f};
        if (p.noise_out) st2(p.noise_out + row * p.noise_rs + j * D + d, ev[j]);
    }

    if (p.iso) {
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            const floatx2 mean = p.c1s * x0v[j] + p.c2s * xtv[j];
            const floatx2 v = (p.noise_mode != 0) ? mean + p.sigs * ev[j] : mean;
            st2x(p.out, rb + j * D + d, p.out_bf16, v);
            if (p.out2) st2(p.out2 + row * p.out2_rs + j * D + d, p.out_bf16 ? __builtin_convertvector(__builtin_convertvector(v, bf16x2), floatx2) : v);
            if (p.mean_out) st2(p.mean_out + row * p.mean_rs + j * D + d, mean);
        }
        return;
    }
    if (p.noise_mode != 0) {
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            ev[j] *= sS[j];
        }
    }
    for (int i = 0; i < J; ++i) {
        floatx2 m1 = {0.f, 0.f}, m2 = {0.f, 0.f}, nz = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            m1 += sC1[i * J + j] * x0v[j];
            m2 += sC2[i * J + j] * xtv[j];
            nz += sU[i * J + j] * ev[j];
        }
        const floatx2 mean = m1 + m2;
        const floatx2 v = (p.noise_mode != 0) ? mean + nz : mean;
        st2x(p.out, rb + i * D + d, p.out_bf16, v);
        // the timages record holds the latent as stored (bf16-rounded in bf16 mode)
        if (p.out2) st2(p.out2 + row * p.out2_rs + i * D + d, p.out_bf16 ? __builtin_convertvector(__builtin_convertvector(v, bf16x2), floatx2) : v);
        if (p.mean_out) st2(p.mean_out + row * p.mean_rs + i * D + d, mean);
    }
}

// Small batches: k_update's thread owns a (row, feature pair) and walks all J nodes serially
// (J Philox draws + 3 J^2 FMAs, ~16 us of dependent work whatever the batch).  Here one
// workgroup per row spreads the same work over (node, feature pair) items in two phases:
//   A: item (j, d): x0 (act, clamp), x_t and sigma_j eps_j of one node -> LDS;
//   B: item (i, d): the C1 / C2 / U sums over j from LDS, in k_update's order and expressions.
__global__ __launch_bounds__(256) void k_update_row(const UpdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int J = p.J, D = p.D, DP = D >> 1, JD = J * D;
    const int nt = p.iso ? 0 : 3 * J * J + J;
    float* sC1 = sm;
    float* sC2 = sC1 + J * J;
    float* sU = sC2 + J * J;
    float* sS = sU + J * J;
    float* sx0 = sm + ((nt + 3) & ~3);
    float* sxt = sx0 + JD;
    float* sev = sxt + JD;
    if (!p.iso) {
        for (int i = threadIdx.x; i < J * J; i += 256) {
            sC1[i] = p.C1[i];
            sC2[i] = p.C2[i];
            sU[i] = p.U[i];
        }
        for (int i = threadIdx.x; i < J; i += 256) sS[i] = p.sig[i];
    }
    const int64_t row = blockIdx.x;
    const int64_t rb = row * (int64_t)JD;
    uint64_t seed = p.seed;
    int64_t row0 = p.row0;
    if (p.noise_mode == 2 && p.rng_dev) {
        seed = p.rng_dev[0];
        row0 = (int64_t)p.rng_dev[1];
    }
    row0 += p.row_shift;
    __syncthreads();  // sS
    for (int q = threadIdx.x; q < J * DP; q += 256) {
        const int j = q / DP, d = 2 * (q - j * DP), o = j * D + d;
        floatx2 a = ld2x(p.x0, rb + o, p.x0_bf16);
        if (p.act == 1) {
            a.x = tanhf(a.x);
            a.y = tanhf(a.y);
        }
        const floatx2 xt = ld2x(p.xt, rb + o, p.xt_bf16);
        if (p.obj) a = start_from_pred(p, xt, a);
        st2(sx0 + o, p.clip ? floatx2{fminf(fmaxf(a.x, -1.f), 1.f), fminf(fmaxf(a.y, -1.f), 1.f)} : a);
        st2(sxt + o, xt);
        floatx2 e;
        if (p.noise_mode == 1) e = ld2(p.eps + row * p.eps_rs + o);
        else if (p.noise_mode == 2) e = noise_pair(seed, (uint64_t)(row0 + row), p.step, (uint32_t)o);
        else e = floatx2{0.f, 0.f};
        if (p.noise_out) st2(p.noise_out + row * p.noise_rs + o, e);
        if (!p.iso && p.noise_mode != 0) e *= sS[j];
        st2(sev + o, e);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < J * DP; q += 256) {
        const int i = q / DP, d = 2 * (q - i * DP), o = i * D + d;
        floatx2 mean, v;
        if (p.iso) {
            mean = p.c1s * ld2(sx0 + o) + p.c2s * ld2(sxt + o);
            v = (p.noise_mode != 0) ? mean + p.sigs * ld2(sev + o) : mean;
        } else {
            floatx2 m1 = {0.f, 0.f}, m2 = {0.f, 0.f}, nz = {0.f, 0.f};
            for (int j = 0; j < J; ++j) {
                m1 += sC1[i * J + j] * ld2(sx0 + j * D + d);
                m2 += sC2[i * J + j] * ld2(sxt + j * D + d);
                nz += sU[i * J + j] * ld2(sev + j * D + d);
            }
            mean = m1 + m2;
            v = (p.noise_mode != 0) ? mean + nz : mean;
        }
        st2x(p.out, rb + o, p.out_bf16, v);
        if (p.out2) st2(p.out2 + row * p.out2_rs + o, p.out_bf16 ? __builtin_convertvector(__builtin_convertvector(v, bf16x2), floatx2) : v);
        if (p.mean_out) st2(p.mean_out + row * p.mean_rs + o, mean);
    }
}

// The posterior update on the matrix cores (J <= 32, D % 16 == 0, nonisotropic).  Per row the
// three J x J projections C1 x0, C2 x_t, U (sigma . eps) are [J x J] x [J x D] products: on
// v_mfma_f32_16x16x4_f32 with A = the coefficient tables (zero-padded to JP, fragments in
// registers) and B = the row's x0 (activation + clamp), x_t and sigma . eps, 16 output columns per
// tile.  The f32 MFMA accumulates its k = 4 products as an fmaf chain in k order
// (MI355X_MICROARCH.md, matrix cores), so over k steps 0 .. JP/4 - 1 each sum is k_update's
// j-ordered fma chain and the result is k_update's bit for bit (zero padding adds exact zeros).
// Workgroup = 4 waves, R rows; wave w takes row w % R and the column tiles w / R, w / R + 4 / R,
// ... (at most MT).  Every x0 / x_t fragment of the wave's tiles is loaded first (16 lanes read 64
// contiguous bytes of one node), so one memory latency covers the whole workgroup; meanwhile the
// tables go to LDS and phase A draws the rows' Philox normals (one 4x32 draw per 4 features, as
// k_noise_fill) into LDS as sigma_j . eps; one barrier; then the MFMAs and the stores.
// BF: x0 / x_t may be bf16 (precision mode 2); the f32 form has no bf16 load path at all (a
// per-operand branch around the loads left the waitcnt pass's merged counts at vmcnt(0))
template <int JP, int R, int MT, bool BF = false>
__global__ __launch_bounds__(256) void k_update_mfma(const UpdArgs p) {
    constexpr int KS = JP / 4, IB = JP / 16;
    // table rows JP + 2 floats apart: an A-fragment read (lanes 0-31 = rows i = l16, k columns l4 in
    // {0, 1}) then hits 32 distinct banks; at a JP stride the 16 rows shared one or two banks (16-way
    // conflicts on every ds_read_b32 of the J <= 64 form, which re-reads its fragments per tile)
    constexpr int TSJ = JP + 2;
    const int J = p.J, D = p.D, JD = J * D, QPR = J * (D >> 2);  // quads per row
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sTab = sm;                        // [3][JP][TSJ] zero-padded C1, C2, U
    // [R][J][D + 16] sigma_j . eps (16-B aligned; the + 16 puts the k columns l4 = 0 / 1 of a B
    // fragment read in different bank halves)
    const int DS = D + 16;
    float* sEv = sm + ((3 * JP * TSJ + 3) & ~3);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t rowg = (int64_t)blockIdx.x * R;
    const int r = wave % R;
    const int64_t row = rowg + r;
    const bool live = row < p.B;  // wave-uniform
    const int64_t rb = (live ? row : 0) * (int64_t)JD;
    const int l16 = lane & 15, l4 = lane >> 4;
    const int nct = D >> 4, ct0 = wave / R, cstep = 4 / R;
    // Order of the prologue's loads (every load of a group issued before its first use: a load ->
    // use loop waits out one memory latency per element).  JP <= 32: the tables, then sigma, then
    // the x0 / x_t fragments, then the table stores (which wait for the tables alone), so the x
    // loads stay in flight through phase A.  JP = 64 (48 table values per thread, which would not
    // fit the registers beside the fragments): sigma, the fragments, then the tables loaded and stored.
    constexpr int TPT = (3 * JP * JP + 255) / 256;
    constexpr bool TFIRST = JP <= 32;
    float tv[TPT];
    auto load_tables = [&]() {
#pragma unroll
        for (int k = 0; k < TPT; ++k) {
            const int q = min(tid + 256 * k, 3 * JP * JP - 1);
            const int m = q / (JP * JP), ij = q % (JP * JP), i = ij / JP, j = ij % JP;
            const float* tab = m == 0 ? p.C1 : m == 1 ? p.C2 : p.U;
            tv[k] = tab[min(i, J - 1) * J + min(j, J - 1)];  // unconditional: padding zeroed at the store
        }
    };
    auto store_tables = [&]() {
#pragma unroll
        for (int k = 0; k < TPT; ++k) {
            const int q = tid + 256 * k;
            const int i = (q % (JP * JP)) / JP, j = q % JP;
            if (q < 3 * JP * JP) sTab[(q / JP) * TSJ + q % JP] = (i < J && j < J) ? tv[k] : 0.f;
        }
    };
    if constexpr (TFIRST) load_tables();
    // sigma_j of this thread's first SGP phase-A quads (unconditional, clamped node)
    constexpr int SGP = 8;
    float sgp[SGP];
    if (p.noise_mode != 0) {  // wave-uniform
#pragma unroll
        for (int it = 0; it < SGP; ++it) sgp[it] = p.sig[min(((tid + 256 * it) % QPR) / (D >> 2), J - 1)];
    }
    // the wave's x0 (activation + clamp) and x_t B fragments, all tiles in flight at once (BF: one
    // uniform branch per operand around all of its loads; a per-element select between the bf16
    // and the f32 load if-converted into both loads plus a merge that waited vmcnt(0) per element)
    float bx[MT][KS], bt[MT][KS];
    auto load_b = [&](const float* src, bool bf16, float (*dst)[KS]) {
        if (BF && bf16) {  // wave-uniform
            const __bf16* sb = reinterpret_cast<const __bf16*>(src);
#pragma unroll
            for (int q = 0; q < MT; ++q)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    dst[q][ks] = (float)sb[rb + min(4 * ks + l4, J - 1) * D + 16 * min(ct0 + q * cstep, nct - 1) + l16];
        } else {
#pragma unroll
            for (int q = 0; q < MT; ++q)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    dst[q][ks] = src[rb + min(4 * ks + l4, J - 1) * D + 16 * min(ct0 + q * cstep, nct - 1) + l16];
        }
    };
    load_b(p.x0, p.x0_bf16, bx);
    load_b(p.xt, p.xt_bf16, bt);
    if constexpr (!TFIRST) load_tables();
    uint64_t seed = p.seed;
    int64_t row0 = p.row0;
    if (p.noise_mode == 2 && p.rng_dev) {
        seed = p.rng_dev[0];
        row0 = (int64_t)p.rng_dev[1];
    }
    row0 += p.row_shift;
    // device noise: the thread's first EPRE draws into registers BEFORE the table stores.  The table
    // stores wait for the table loads, and with every workgroup's fragment loads in flight those took
    // ~4 us (stamps, profiles/r05d/update_stamps.txt) -- the Philox work (~3 us) now runs under that wait
    // instead of after it.  Same draws, same scaling below: the same bits.
    constexpr int EPRE = (R * JP * 24 + 255) / 256 < SGP ? (R * JP * 24 + 255) / 256 : SGP;
    floatx4 epre[EPRE];
    if (p.noise_mode == 2) {  // wave-uniform
#pragma unroll
        for (int it = 0; it < EPRE; ++it) {
            const int q = min(tid + 256 * it, R * QPR - 1);  // clamped: a spare draw is never used
            const int rr = q / QPR, qq = q % QPR;
            const uint4 x = philox_at(seed, (uint64_t)(row0 + rowg + rr), p.step, (uint32_t)qq);
            const floatx2 z0 = box_muller(x.x, x.y), z1 = box_muller(x.z, x.w);
            epre[it] = floatx4{z0.x, z0.y, z1.x, z1.y};
        }
    }
    store_tables();
    // phase A: sigma_j eps_j (and the raw eps record) for the workgroup's rows (the first SGP
    // quads' sigma_j prefetched above: loaded in the loop, each was waited out right away).  One
    // loop per noise mode (a wave-uniform branch around whole loops): with the given-noise load and
    // the Philox draw as two arms of one body, the waitcnt pass merged the arms and waited
    // vmcnt(0) -- every x0 / x_t fragment load above -- before the first draw was even scaled
    // it: the item's index among this thread's first SGP items (its draw may be in epre), -1 beyond
    auto phase_a = [&](auto nm, int q, float sg, int it) {
        constexpr int NM = decltype(nm)::value;
        const int rr = q / QPR, qq = q % QPR, j = qq / (D >> 2), d = 4 * (qq % (D >> 2));
        const int64_t rw = rowg + rr;
        if (rw >= p.B) return;
        floatx4 e = {0.f, 0.f, 0.f, 0.f};
        if constexpr (NM == 1) {
            e = ld4(p.eps + rw * p.eps_rs + j * D + d);
        } else if constexpr (NM == 2) {
            if (it >= 0 && it < EPRE) {  // compile-time after unrolling
                e = epre[it < EPRE ? it : 0];
            } else {
                const uint4 x = philox_at(seed, (uint64_t)(row0 + rw), p.step, (uint32_t)qq);
                const floatx2 z0 = box_muller(x.x, x.y), z1 = box_muller(x.z, x.w);
                e = floatx4{z0.x, z0.y, z1.x, z1.y};
            }
        }
        if (p.noise_out) *reinterpret_cast<floatx4*>(p.noise_out + rw * p.noise_rs + j * D + d) = e;
        if constexpr (NM != 0) e *= sg;
        *reinterpret_cast<floatx4*>(sEv + (rr * J + j) * DS + d) = e;
    };
    auto run_a = [&](auto nm) {
#pragma unroll
        for (int it = 0; it < SGP; ++it)
            if (tid + 256 * it < R * QPR) phase_a(nm, tid + 256 * it, sgp[it], it);
        for (int q = tid + 256 * SGP; q < R * QPR; q += 256)
            phase_a(nm, q, decltype(nm)::value != 0 ? p.sig[(q % QPR) / (D >> 2)] : 1.f, -1);
    };
    if (p.noise_mode == 2) run_a(std::integral_constant<int, 2>{});
    else if (p.noise_mode == 1) run_a(std::integral_constant<int, 1>{});
    else run_a(std::integral_constant<int, 0>{});
    __syncthreads();
    if (!live) return;  // wave-uniform; no barrier follows
    // A fragments: lane (l16, l4) holds table[i = 16 ib + l16][j = 4 ks + l4]; JP <= 32: every
    // output block's fragments in registers for the whole row, JP = 64 (J <= 64): one block's at a
    // time, re-read from LDS per column tile (3 x 16 x 4 fragments would not fit the registers)
    constexpr bool AREG = JP <= 32;
    float A[3][AREG ? IB : 1][KS];
    auto load_a = [&](int ib, int slot) {
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) A[m][slot][ks] = sTab[(m * JP + 16 * ib + l16) * TSJ + 4 * ks + l4];
    };
    if constexpr (AREG) {
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) load_a(ib, ib);
    }
    // activation + clamp of every tile's x0 first: tanhf branches per lane, and with that
    // divergent code between one tile's stores and the next tile's work the waitcnt pass drained
    // vmcnt(0) -- the previous tile's stores -- once per tile
#pragma unroll
    for (int q = 0; q < MT; ++q)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float a = bx[q][ks];
            if (p.act == 1) a = tanhf(a);
            bx[q][ks] = p.clip ? fminf(fmaxf(a, -1.f), 1.f) : a;
        }
    // every tile's result first, then the stores back to back: with a tile's stores between its
    // MFMAs and the next tile's, the next tile reused the pending stores' data / address registers
    // and the waitcnt pass drained vmcnt(0) -- one store round trip -- per tile (15 such waits)
    floatx4 vres[MT][IB];
#pragma unroll
    for (int q = 0; q < MT; ++q) {
        const int ct = ct0 + q * cstep;
        if (ct >= nct) continue;  // wave-uniform
        const int n = 16 * ct + l16;
        float bxa[KS], bta[KS], be[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int j = 4 * ks + l4;
            const bool ok = j < J;
            bxa[ks] = ok ? bx[q][ks] : 0.f;
            bta[ks] = ok ? bt[q][ks] : 0.f;
            be[ks] = ok ? sEv[(r * J + j) * DS + n] : 0.f;
        }
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) {
            if (16 * ib >= J) continue;  // wave-uniform: an output block of padding only
            const int sl = AREG ? ib : 0;
            if constexpr (!AREG) load_a(ib, 0);
            // D^T = X^T Tab^T: A = the row's x0 / x_t / sigma eps fragment, B = the table's, so
            // D[n = 16 ct + 4 l4 + e][i = 16 ib + l16] -- four consecutive features of one node
            // per lane, 16-B stores (the same fmaf chain over j as Tab X: fmaf is symmetric)
            floatx4 m1 = {0.f, 0.f, 0.f, 0.f}, m2 = m1, nz = m1;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                m1 = __builtin_amdgcn_mfma_f32_16x16x4f32(bxa[ks], A[0][sl][ks], m1, 0, 0, 0);
                m2 = __builtin_amdgcn_mfma_f32_16x16x4f32(bta[ks], A[1][sl][ks], m2, 0, 0, 0);
                nz = __builtin_amdgcn_mfma_f32_16x16x4f32(be[ks], A[2][sl][ks], nz, 0, 0, 0);
            }
            const floatx4 mean = m1 + m2;
            vres[q][ib] = (p.noise_mode != 0) ? mean + nz : mean;
            const int i = 16 * ib + l16;
            if (p.mean_out && i < J)  // records only (the mean_t record of sample_loop)
                *reinterpret_cast<floatx4*>(p.mean_out + row * p.mean_rs + i * D + 16 * ct + 4 * l4) = mean;
        }
    }
#pragma unroll
    for (int q = 0; q < MT; ++q) {
        const int ct = ct0 + q * cstep;
        if (ct >= nct) continue;  // wave-uniform
        const int n4 = 16 * ct + 4 * l4;
#pragma unroll
        for (int ib = 0; ib < IB; ++ib) {
            const int i = 16 * ib + l16;
            if (16 * ib >= J || i >= J) continue;
            const floatx4 v = vres[q][ib];
            const int64_t o = rb + i * D + n4;
            if (p.out_bf16) {
                const bf16x4 vb = __builtin_convertvector(v, bf16x4);
                *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(p.out) + o) = vb;
                if (p.out2) *reinterpret_cast<floatx4*>(p.out2 + row * p.out2_rs + i * D + n4) = __builtin_convertvector(vb, floatx4);
            } else {
                *reinterpret_cast<floatx4*>(p.out + o) = v;
                if (p.out2) *reinterpret_cast<floatx4*>(p.out2 + row * p.out2_rs + i * D + n4) = v;
            }
        }
    }
}

// rows at or below which launch_update runs k_update_row
constexpr int64_t kUpdateRows = 1024;

hipError_t launch_update(const UpdArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    // k_update_mfma where it applies, unless the plan asks for the element-per-thread forms
    // (SD_OPT_UPDATE_KERNEL; both give the same bits)
    const bool g_update_mfma = !a.elementwise;
    // the wave's column tiles (all of them in flight): D / 16 tiles over 4 / R waves, at most 6
    const int Rm = a.B <= kUpdateRows ? 1 : 4;
    if (g_update_mfma && !a.iso && a.J > 32 && a.J <= 64 && a.D % 16 == 0 && (a.D / 16 + 3) / 4 <= 2) {
        // J <= 64 (MANO J = 51 / 52): one row per workgroup, each wave at most two column tiles
        const size_t lds = (((3 * 64 * 66 + 3) & ~(size_t)3) + (size_t)a.J * (a.D + 16)) * sizeof(float);
        if (lds > kLdsMax) return hipErrorNotSupported;
        auto kern = (a.x0_bf16 || a.xt_bf16) ? k_update_mfma<64, 1, 2, true> : k_update_mfma<64, 1, 2>;
        if (const hipError_t e = lds_opt_in(kern, lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)a.B), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    // the instantiations below cover MT column tiles per wave, cstep = 4 / R apart: R = 1 -> MT = 2
    // (tiles w, w + 4: D <= 128), R = 4 -> MT = 6 (tiles 0..5: D <= 96); wider rows take the forms below
    if (g_update_mfma && !a.iso && a.J <= 32 && a.D % 16 == 0 && a.D / 16 <= (Rm == 1 ? 8 : 6)) {
        // small batches: one row per workgroup (4 waves share its column tiles), else 4 rows
        const int R = Rm;
        const dim3 grid((unsigned)((a.B + R - 1) / R));
        auto go = [&](auto kern, int JP) -> hipError_t {
            const size_t lds = (((3 * (size_t)JP * (JP + 2) + 3) & ~(size_t)3) + (size_t)R * a.J * (a.D + 16)) * sizeof(float);
            if (lds > kLdsMax) return hipErrorNotSupported;
            if (const hipError_t e = lds_opt_in(kern, lds); e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
            return hipGetLastError();
        };
        const bool bf = a.x0_bf16 || a.xt_bf16;
        if (a.J <= 16)
            return R == 1 ? go(bf ? k_update_mfma<16, 1, 2, true> : k_update_mfma<16, 1, 2>, 16)
                          : go(bf ? k_update_mfma<16, 4, 6, true> : k_update_mfma<16, 4, 6>, 16);
        return R == 1 ? go(bf ? k_update_mfma<32, 1, 2, true> : k_update_mfma<32, 1, 2>, 32)
                      : go(bf ? k_update_mfma<32, 4, 6, true> : k_update_mfma<32, 4, 6>, 32);
    }
    if (a.B <= kUpdateRows && a.D % 2 == 0) {
        const size_t nt = a.iso ? 0 : 3 * (size_t)a.J * a.J + a.J;
        const size_t lds = (((nt + 3) & ~(size_t)3) + 3 * (size_t)a.J * a.D) * sizeof(float);
        if (lds <= kLdsDefault) {
            hipLaunchKernelGGL(k_update_row, dim3((unsigned)a.B), dim3(256), lds, s, a);
            return hipGetLastError();
        }
    }
    const int64_t n = a.B * (a.D / 2);
    const dim3 grid((unsigned)((n + 255) / 256));
    switch (a.J) {
        case 16: hipLaunchKernelGGL((k_update<16, true>), grid, dim3(256), 0, s, a); break;
        case 17: hipLaunchKernelGGL((k_update<17, true>), grid, dim3(256), 0, s, a); break;
        case 21: hipLaunchKernelGGL((k_update<21, true>), grid, dim3(256), 0, s, a); break;
        case 51: hipLaunchKernelGGL((k_update<51, true>), grid, dim3(256), 0, s, a); break;
        default:
            if (a.J <= 16) hipLaunchKernelGGL((k_update<16, false>), grid, dim3(256), 0, s, a);
            else if (a.J <= 32) hipLaunchKernelGGL((k_update<32, false>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_update<64, false>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// =============================================================================================
// One-time plan helpers
// =============================================================================================

// SinusoidalPosEmb (denoising_diffusion_pytorch 1.9.4, restated): emb[t] = [sin(t f), cos(t f)],
// f_k = exp(k * neg_scale), neg_scale = -ln(theta)/(half-1) rounded to fp32 as torch does.
__global__ void k_sinusoidal(float* emb, int T, int dim, float neg_scale) {
    const int half = dim / 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T * half) return;
    const int t = g / half, k = g % half;
    const float f = expf((float)k * neg_scale);
    const float a = (float)t * f;
    emb[t * dim + k] = sinf(a);
    emb[t * dim + half + k] = cosf(a);
}

hipError_t launch_sinusoidal(float* emb, int T, int dim, float neg_scale, hipStream_t s) {
    const int n = T * (dim / 2);
    hipLaunchKernelGGL(k_sinusoidal, dim3((n + 255) / 256), dim3(256), 0, s, emb, T, dim, neg_scale);
    return hipGetLastError();
}

// y[m][n] = out_act( sum_k in_act(x[m][k]) W[n][k] + b[n] ); in_act 1 = tanh, out_act 1 = GELU(erf)
__global__ void k_linear(const float* x, int M, int K, const float* W, const float* b, int N,
                         float* y, int in_act, int out_act) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= M * N) return;
    const int m = g / N, n = g % N;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        float v = x[m * K + k];
        if (in_act == 1) v = tanhf(v);
        acc = fmaf(v, W[(int64_t)n * K + k], acc);
    }
    if (b) acc += b[n];
    if (out_act == 1) acc = 0.5f * acc * (1.0f + erff(acc * 0.70710678118654752f));
    y[g] = acc;
}

hipError_t launch_linear(const float* x, int M, int K, const float* W, const float* b, int N,
                         float* y, int in_act, int out_act, hipStream_t s) {
    const int n = M * N;
    hipLaunchKernelGGL(k_linear, dim3((n + 255) / 256), dim3(256), 0, s, x, M, K, W, b, N, y,
                       in_act, out_act);
    return hipGetLastError();
}

// G-hat = F.normalize(G, p=1, dim=1) (row-L1, graph_structural.py:31-32) or G unchanged.
__global__ void k_ghat(const float* G, float* Gh, int J, int normalize) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= J) return;
    float s = 0.f;
    for (int j = 0; j < J; ++j) s += fabsf(G[i * J + j]);
    const float den = fmaxf(s, 1e-12f);
    for (int j = 0; j < J; ++j) Gh[i * J + j] = normalize ? G[i * J + j] / den : G[i * J + j];
}

hipError_t launch_ghat(const float* G, float* Ghat, int J, int normalize, hipStream_t s) {
    hipLaunchKernelGGL(k_ghat, dim3(1), dim3(64), 0, s, G, Ghat, J, normalize);
    return hipGetLastError();
}

// RMSNorm gain folded into the following projection: W'[r][k] = W[r][k] * (g[k] * mult)
__global__ void k_fold_gain(const float* W, const float* g, float mult, float* out, int64_t rows, int K) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * K) return;
    out[i] = W[i] * (g[i % K] * mult);
}

hipError_t launch_fold_gain(const float* W, const float* g, float mult, float* out, int64_t rows,
                            int K, hipStream_t s) {
    const int64_t n = rows * K;
    hipLaunchKernelGGL(k_fold_gain, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, g, mult,
                       out, rows, K);
    return hipGetLastError();
}

// sigma_t = exp(0.5 * log_variance_clipped)   (nonisotropic.py:210)
__global__ void k_sigma(const float* lv, float* sig, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sig[i] = expf(0.5f * lv[i]);
}

hipError_t launch_sigma(const float* logvar, float* sig, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_sigma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logvar, sig, n);
    return hipGetLastError();
}

}  // namespace sd

