// StaticGraphLinear (graph_structural.py:30-43) + fused epilogue: the dispatcher over the kernel
// generations (launch_graph_linear, at the end) and k_gl2, the v2 schedule for gfx950 -- the exact-f32
// kernel every other generation falls through to.
//
// k_gl2's tile.  Workgroup = 4 waves; a wave owns 16 rows x (16*NCB) output columns for ALL J nodes,
// so the G-hat node mixing (which couples the J nodes of a row) and the epilogue run in registers.
// The per-node GEMM is on the exact-f32 MFMA v_mfma_f32_16x16x4_f32, operand maps
// (cdna_hip_programming.md §3): lane l supplies A[l&15][k=l>>4] and B[k=l>>4][l&15];
// D[row=4*(l>>4)+r][col=l&15].  k is permuted inside a 16-wide chunk so each lane reads ONE float4 of
// x and ONE float4 of W per 4 MFMAs: in step s of chunk kc, position p = l>>4 carries k = kc + 4p + s
// for both operands.
// How the operands arrive:
//   * the weight tile of a 16-deep k chunk (all node types x 16*NCB columns) is brought into LDS
//     ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4, no VGPRs), double-buffered, and
//     shared by the 4 waves;
//   * LDS image [type][k-group][n][4 floats]: the 16 lanes of every ds_read_b128 lane group
//     read 16 distinct consecutive 16-B slots -> conflict-free;
//   * each node's x fragment for chunk c+1 is issued right after its last use in chunk c, so the
//     global latency hides under the other J-1 nodes' MFMAs (small J; large J loads on demand);
//   * __launch_bounds__(256, 2): <= 256 VGPR+AGPR, two workgroups per CU.
// One barrier per chunk: it retires the DMA for the next stage (RAW) and frees the stage the
// next fill overwrites (WAR).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sd_device.h"
#include "sd_gl4_args.h"
#include "sd_internal.h"

namespace sd {

thread_local unsigned g_route_bits = 0;

namespace {

template <int NT>
__device__ __forceinline__ void fill_w_stage(const GLArgs& p, int c0, int k0, int K, float* dst, int wave,
                                             int lane) {
    // piece q (16 B) = (type, k-group, n), n fastest; one wave instruction = 64 pieces = 1 KiB
    const int npieces = p.ntypes * 4 * NT;
    for (int q0 = wave * 64; q0 < npieces; q0 += 256) {
        const int q = q0 + lane;
        const int n = q % NT;
        const int tl = q / NT;
        const int col = min(c0 + n, p.N - 1);  // tail columns: any valid row, never stored
        const float* src = p.W + ((int64_t)(tl >> 2) * p.N + col) * K + k0 + 4 * (tl & 3);
        __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)(dst + (size_t)q0 * 4), 16, 0, 0);
    }
}

}  // namespace

template <int JM, bool EXACT, int NCB, bool RMS, bool PREF, int MINW>
__global__ __launch_bounds__(256, MINW) void k_gl2(const GLArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = 16 * NCB;
    const int J = EXACT ? JM : p.J;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int stage = p.ntypes * NT * 16;
    float* sW0 = smem;
    float* sW1 = smem + stage;
    float* sG = smem + 2 * stage;

    // XCD-aware tile order: the column tiles of one row tile, which re-read the same x rows, stay
    // inside one XCD's L2
    const int ntile_c = (p.N + NT - 1) / NT;
    const int L = (int)xcd_remap(blockIdx.x, gridDim.x >> 3, gridDim.x & 7);
    const int ct = L % ntile_c;
    const int64_t rt = L / ntile_c;
    const int64_t row0 = rt * 64 + wave * 16;
    const int c0 = ct * NT;
    const int K = p.K1 + p.K2;
    const int nchunk = K >> 4;

    const int64_t arow = row0 + lr;
    const bool rok = arow < p.B;
    const int64_t arow_c = rok ? arow : 0;
    const float* x1r = p.x1 + ((arow_c + p.x1_row0) / p.x1_div) * p.x1_rs + 4 * lg;
    const float* x2r = p.K2 ? p.x2 + arow_c * p.x2_rs + 4 * lg : nullptr;
    // Tail rows read row 0 (valid memory) and are never stored, so every wave issues exactly J
    // x loads per chunk - the counted vmcnt below relies on that count.
    auto load_a = [&](int c, int j) -> floatx4 {
        const int k0 = c << 4;
        const float* src = (k0 < p.K1) ? x1r + (int64_t)j * p.K1 + k0 : x2r + (int64_t)j * p.K2 + (k0 - p.K1);
        return ld4(src);
    };

    floatx4 acc[JM][NCB];
    floatx4 a[JM];
    float ss[JM];
#pragma unroll
    for (int j = 0; j < JM; ++j) {
        ss[j] = 0.f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[j][cb] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

    fill_w_stage<NT>(p, c0, 0, K, sW0, wave, lane);
    for (int i = tid; i < J * J; i += 256) sG[i] = p.G[i];
    if (PREF) {
#pragma unroll
        for (int j = 0; j < JM; ++j)
            if (EXACT || j < J) a[j] = load_a(0, j);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int c = 0; c < nchunk; ++c) {
        const float* cur = (c & 1) ? sW1 : sW0;
        if (c + 1 < nchunk) fill_w_stage<NT>(p, c0, (c + 1) << 4, K, (c & 1) ? sW0 : sW1, wave, lane);
        const bool rms_chunk = RMS && (c << 4) < p.K1;
        const int cn = min(c + 1, nchunk - 1);  // branch-free prefetch (last chunk re-reads itself)
        // B fragments are read one node ahead so the ds_read latency hides under the MFMAs
        floatx4 bnext[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
            bnext[cb] = *reinterpret_cast<const floatx4*>(cur + ((p.ntype[0] * 4 + lg) * NT + lr) * 4 + cb * 64);
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            floatx4 bj[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) bj[cb] = bnext[cb];
            if (j + 1 < JM && (EXACT || j + 1 < J)) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
                    bnext[cb] = *reinterpret_cast<const floatx4*>(
                        cur + ((p.ntype[j + 1] * 4 + lg) * NT + lr) * 4 + cb * 64);
            }
            floatx4 aj;
            if (PREF) {
                aj = a[j];
                a[j] = load_a(cn, j);
            } else {
                aj = load_a(c, j);
            }
            if (rms_chunk) ss[j] += aj.x * aj.x + aj.y * aj.y + aj.z * aj.z + aj.w * aj.w;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const floatx4 b = bj[cb];
                floatx4 cc = acc[j][cb];
                cc = mfma4(aj.x, b.x, cc);
                cc = mfma4(aj.y, b.y, cc);
                cc = mfma4(aj.z, b.z, cc);
                cc = mfma4(aj.w, b.w, cc);
                acc[j][cb] = cc;
            }
        }
        bool counted = false;
        if constexpr (PREF && EXACT) {
            if (c + 1 < nchunk) {
                // Issue order in this chunk: weight DMA for c+1 first, then the J x prefetches
                // for c+1.  vmcnt(J) retires the DMA while leaving the x loads in flight across
                // the barrier (a __syncthreads() would emit vmcnt(0) and drain them).
                __builtin_amdgcn_s_waitcnt(VmCnt<JM>::imm);
                __builtin_amdgcn_s_barrier();
                counted = true;
            }
        }
        if (!counted) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }

    if (row0 >= p.B) return;  // no barrier below
    if (RMS) {  // F.normalize(x, dim=-1): 1 / max(||x_bj||, 1e-12) per (row, node)
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            float t = ss[j];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = 1.0f / fmaxf(sqrtf(__shfl(t, 4 * lg + r)), 1e-12f);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[j][cb][r] *= s;
            }
        }
    }
    if (p.bias) {  // per source node, before the mixing (graph_structural.py:38-41)
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int n = c0 + 16 * cb + lr;
                acc[j][cb] += (n < p.N) ? p.bias[p.wrow[j] + n] : 0.f;
            }
        }
    }
    float fa[NCB], fb[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int n = c0 + 16 * cb + lr;
        fa[cb] = 1.f;
        fb[cb] = 0.f;
        if (p.film && n < p.N) {
            fa[cb] = p.film[n] + 1.0f;
            fb[cb] = p.film[p.N + n];
        }
    }
    for (int i = 0; i < J; ++i) {
        floatx4 z[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) z[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < JM; ++j) {
            if (!EXACT && j >= J) continue;
            const float g = sG[i * J + j];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) z[cb] += g * acc[j][cb];
        }
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int n = c0 + 16 * cb + lr;
            if (n >= p.N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 4 * lg + r;
                if (row >= p.B) continue;
                float v = z[cb][r];
                if (p.film) v = v * fa[cb] + fb[cb];
                if (p.act == 1) v = tanhf(v);
                if (p.res) v += p.res[row * p.res_rs + (int64_t)i * p.N + n];
                p.out[row * p.out_rs + (int64_t)i * p.N + n] = v;
            }
        }
    }
}

template <int JM, bool EXACT, int NCB, bool PREF, int MINW>
static hipError_t gl2_launch(const GLArgs& a, bool rms, hipStream_t s) {
    constexpr int NT = 16 * NCB;
    const int ntile_c = (a.N + NT - 1) / NT;
    const int64_t ntile_r = (a.B + 63) / 64;
    const dim3 grid((unsigned)(ntile_c * ntile_r));
    size_t lds = (size_t)(2 * a.ntypes * NT * 16 + a.J * a.J) * sizeof(float);
    if (lds > kLdsMax) return hipErrorInvalidValue;
    auto kt = rms ? k_gl2<JM, EXACT, NCB, true, PREF, MINW> : k_gl2<JM, EXACT, NCB, false, PREF, MINW>;
    if (const hipError_t e = lds_opt_in(kt, lds); e != hipSuccess) return e;
    g_route_bits |= kRouteExact;
    hipLaunchKernelGGL(kt, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

// Column-tile width: 32 (NCB=2) halves the x re-reads, 16 (NCB=1) doubles the number of
// workgroups; at small B*N the 32-wide grid cannot give every CU two workgroups, so go narrow.
static int ncb_choice(const GLArgs& a) {
    const int64_t wgs32 = (int64_t)((a.N + 31) / 32) * ((a.B + 63) / 64);
    return wgs32 >= 2 * 256 ? 2 : 1;
}

hipError_t launch_graph_linear_v2(const GLArgs& a, bool rms, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    // two 32-column weight stages must fit comfortably in LDS
    const bool wide = ncb_choice(a) == 2 && a.ntypes * 32 * 16 * 4 * 2 <= 96 * 1024;
    switch (a.J) {
        case 16: return wide ? gl2_launch<16, true, 2, true, 2>(a, rms, s) : gl2_launch<16, true, 1, true, 3>(a, rms, s);
        case 17: return wide ? gl2_launch<17, true, 2, true, 2>(a, rms, s) : gl2_launch<17, true, 1, true, 3>(a, rms, s);
        case 21: return gl2_launch<21, true, 1, true, 2>(a, rms, s);
        case 51: return gl2_launch<51, true, 1, false, 1>(a, rms, s);
        default: break;
    }
    if (a.J <= 8) return gl2_launch<8, false, 2, true, 2>(a, rms, s);
    if (a.J <= 16) return gl2_launch<16, false, 1, true, 2>(a, rms, s);
    if (a.J <= 32) return gl2_launch<32, false, 1, false, 2>(a, rms, s);
    return gl2_launch<64, false, 1, false, 1>(a, rms, s);
}

// 0 (default): v4 (f32-accurate split-f16 MFMA) where the plan prepared split weights and the
// skeleton has an instantiation; otherwise the exact-f32 kernels per shape: v3 (node-split
// waves, 32x32 f32 MFMA) for N < 512, where it measured 1.15-1.25x faster than v2; v2 with
// 32-column tiles for the wide to_qkv layer (N = 768); v5 (node-batched GEMM + mixing pass) for
// J > 21, where every one-kernel tile must stage all node types' weights.  2..5 force one
// generation (falling through to v2 where the forced one does not apply); 1, the removed first
// generation, is an alias of 2.
hipError_t launch_graph_linear(const GLArgs& a, bool rms, hipStream_t s) {
    const int v = a.variant;
    // every generation computes a column tile from the whole K extent of its rows: an input that
    // aliases the output would be overwritten by sibling column tiles while still being read
    if (a.B > 0 && (a.x1 == a.out || (a.x2 && a.x2 == a.out))) return hipErrorInvalidValue;
    if (a.skip_mix) return (v == 0 || v == 5) && a.J > 21 && a.prec != 2 ? launch_graph_linear_v5(a, rms, s) : hipErrorNotSupported;
    // Block.norm 'layer' lives in the v4 mixing epilogue only (J = 16 / 17 / 21; plan-time checked)
    if (a.ln_w) return v == 0 || v == 4 ? launch_graph_linear_v4(a, rms, s) : hipErrorNotSupported;
    if (v == 4 || v == 0) {
        const hipError_t e = launch_graph_linear_v4(a, rms, s);
        if (e != hipErrorNotSupported) return e;
    }
    // bf16 operands (precision mode 2) exist only in the v4 tiles: no exact-f32 fallback
    if (a.prec == 2 || a.x1_bf16 || a.x2_bf16 || a.res_bf16 || a.out_bf16) return hipErrorNotSupported;
    // the exact-f32 generations read and write row-major activations only
    if (a.x1_blk || a.x2_blk || a.res_blk || a.out_blk) return hipErrorNotSupported;
    // large skeletons (J > 21, MANO J = 51: 43 node types): node-batched GEMM + mixing pass
    if (v == 5 || (v == 0 && a.J > 21)) {
        const hipError_t e = launch_graph_linear_v5(a, rms, s);
        if (e != hipErrorNotSupported) return e;
    }
    if (v == 3 || (v == 0 && a.N < 512)) {
        const hipError_t e = launch_graph_linear_v3(a, rms, s);
        if (e != hipErrorNotSupported) return e;
    }
    return launch_graph_linear_v2(a, rms, s);
}

}  // namespace sd
