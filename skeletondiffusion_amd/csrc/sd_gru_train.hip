// Training side of the graph-GRU: the recurrent core of StaticGraphGRUCell
// (src/core/network/layers/recurrent.py:321-366, clockwork off) over a whole sequence with the
// state backward needs, its backward through time, and the gx table with a backward
// (recurrent.py:361-364).  Notation of sd_decoder.hip; per batch row and step t:
//   c_t  = W_hh[type j] h_{t-1} + b_hh[type j]                       (J, 3H), unmixed
//   X_t  = gx_t a_t,  Hh_t = gx_t c_t                                a_t = W_ih x_t + b_ih, unmixed
//   r = sigma(X_r + Hh_r), z = sigma(X_z + Hh_z), n = tanh(X_n + r Hh_n),  h_t = n - n z + z h_{t-1}
// Launch structure (the batch is 64 rows: a persistent workgroup per row tile would hold 2-4 CUs):
//   forward, per step:  k_gru_hh (c_t, one workgroup per (node, 8 rows)), k_gru_gate (mix + gates)
//   backward, per step: k_gru_gate_bwd (dP_t = [pr | pz | pn | pn r], carry dh z),
//                       k_gru_bwd_hh (dc_t = gx_t^T dHh_t, dh_{t-1} = carry + W_hh^T dc_t)
//   after the reverse sweep, over all B T rows at once: da = gx^T dX (k_gru_da), dW_hh / db_hh
//   (the per-type GEMM and bias reduction of sd_gl_train_backward on x = h_{t-1}, dy = dc with an
//   identity mixing matrix), dgx = sum_b (dX a^T + dHh c^T) (k_gru_dgx_part + k_seq_dgx_sum).
// Every reduction over rows and steps runs in a fixed order (no float atomics): two runs give
// the same bits.  The gate math is sd_gru_gates.h, shared with the host emulation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_gru_gates.h"
#include "sd_internal.h"

namespace sd {
namespace {

#include "sd_seq_train.h"

constexpr int kGruMaxH = kSeqMaxH;        // hidden width the per-step kernels' LDS tiles are sized for
constexpr int kGruRT = kSeqRT;            // rows per workgroup of k_gru_hh / k_gru_bwd_hh
constexpr int kGruCH = 16;                // hidden features per workgroup of k_gru_gate (H % 16 == 0)
constexpr int kGruDgxRows = kSeqDgxRows;  // rows per partial of the dgx reduction

// W (types, 3H, H) -> Wt (types, H, 3H): k_gru_hh reads unit-stride over the output column
__global__ void k_gru_transpose_w(const float* __restrict__ W, int64_t types, int H, float* __restrict__ Wt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int H3 = 3 * H;
    if (e >= types * H3 * H) return;
    const int64_t t = e / ((int64_t)H3 * H);
    const int rem = (int)(e % ((int64_t)H3 * H));
    const int k = rem / H3, n = rem % H3;
    Wt[e] = W[(t * H3 + n) * H + k];
}

// dst (rows, J H) contiguous <- src rows at stride src_rs
__global__ void k_gru_copy_rows(const float* __restrict__ src, int64_t src_rs, float* __restrict__ dst, int64_t dst_rs,
                                int64_t rows, int n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * n) return;
    const int64_t r = e / n;
    const int k = (int)(e % n);
    dst[r * dst_rs + k] = src[r * src_rs + k];
}

// c[b, j, :] = W_hh[type j] h[b, j, :] + b_hh[type j] for node j = blockIdx.x and the kGruRT rows
// from blockIdx.y * kGruRT: the rows' h in LDS (16-B broadcast reads), thread -> output column n,
// Wt unit-stride over n.  h / c rows at strides h_rs / c_rs (slabs of (B, T, J, .) tensors).
__global__ __launch_bounds__(1024) void k_gru_hh(const float* __restrict__ h, int64_t h_rs, const float* __restrict__ Wt,
                                                 const float* __restrict__ bias, NodeTypes nt, float* __restrict__ c,
                                                 int64_t c_rs, int64_t B, int J, int H) {
    __shared__ __attribute__((aligned(16))) float sh[kGruRT][kGruMaxH];
    const int j = blockIdx.x, H3 = 3 * H;
    const int64_t b0 = (int64_t)blockIdx.y * kGruRT;
    const int t = nt.t[j];
    for (int e = threadIdx.x; e < kGruRT * H; e += blockDim.x) {
        const int r = e / H, k = e - r * H;
        sh[r][k] = b0 + r < B ? h[(b0 + r) * h_rs + (int64_t)j * H + k] : 0.f;
    }
    __syncthreads();
    const float* W = Wt + (int64_t)t * H * H3;
    for (int n = threadIdx.x; n < H3; n += blockDim.x) {
        float acc[kGruRT];
        const float bv = bias ? bias[(int64_t)t * H3 + n] : 0.f;
#pragma unroll
        for (int r = 0; r < kGruRT; ++r) acc[r] = bv;
        for (int k = 0; k < H; k += 4) {
            const float w0 = W[(int64_t)k * H3 + n], w1 = W[(int64_t)(k + 1) * H3 + n];
            const float w2 = W[(int64_t)(k + 2) * H3 + n], w3 = W[(int64_t)(k + 3) * H3 + n];
#pragma unroll
            for (int r = 0; r < kGruRT; ++r) {
                const float4 hv = *reinterpret_cast<const float4*>(&sh[r][k]);
                acc[r] = fmaf(w0, hv.x, acc[r]);
                acc[r] = fmaf(w1, hv.y, acc[r]);
                acc[r] = fmaf(w2, hv.z, acc[r]);
                acc[r] = fmaf(w3, hv.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kGruRT; ++r)
            if (b0 + r < B) c[(b0 + r) * c_rs + (int64_t)j * H3 + n] = acc[r];
    }
}

// One workgroup per (row b, kGruCH hidden features): the three gate column groups of a_t[b] and
// c_t[b] for those features and gx_t in LDS; thread -> (node i, feature) mixes both over the nodes
// and applies the gates.  Writes h_t to hs (and to the next step's h_prev slab and the gate record
// when state is kept).
__global__ __launch_bounds__(256) void k_gru_gate(const float* __restrict__ a, int64_t a_rs, const float* __restrict__ c,
                                                  int64_t c_rs, const float* __restrict__ gx,
                                                  const float* __restrict__ hprev, int64_t hp_rs, float* __restrict__ hs,
                                                  int64_t hs_rs, float* __restrict__ hnext, int64_t hn_rs,
                                                  float* __restrict__ gates, int64_t g_rs, int J, int H) {
    __shared__ float sa[kMaxNodes][3 * kGruCH];
    __shared__ float sc[kMaxNodes][3 * kGruCH];
    __shared__ float sg[kMaxNodes][kMaxNodes + 1];
    const int64_t b = blockIdx.x;
    const int c0 = blockIdx.y * kGruCH, H3 = 3 * H;
    for (int e = threadIdx.x; e < J * 3 * kGruCH; e += 256) {
        const int j = e / (3 * kGruCH), q = e - j * 3 * kGruCH;
        const int col = (q / kGruCH) * H + c0 + (q % kGruCH);
        sa[j][q] = a[b * a_rs + (int64_t)j * H3 + col];
        sc[j][q] = c[b * c_rs + (int64_t)j * H3 + col];
    }
    for (int e = threadIdx.x; e < J * J; e += 256) sg[e / J][e % J] = gx[e];
    __syncthreads();
    for (int o = threadIdx.x; o < J * kGruCH; o += 256) {
        const int i = o / kGruCH, cc = o % kGruCH;
        float xr = 0.f, xz = 0.f, xn = 0.f, hr = 0.f, hz = 0.f, hn = 0.f;
        for (int j = 0; j < J; ++j) {
            const float g = sg[i][j];
            xr = fmaf(g, sa[j][cc], xr);
            xz = fmaf(g, sa[j][kGruCH + cc], xz);
            xn = fmaf(g, sa[j][2 * kGruCH + cc], xn);
            hr = fmaf(g, sc[j][cc], hr);
            hz = fmaf(g, sc[j][kGruCH + cc], hz);
            hn = fmaf(g, sc[j][2 * kGruCH + cc], hn);
        }
        const int64_t ih = (int64_t)i * H + c0 + cc;
        const gru::GateFwd<float> f = gru::gate_forward(xr, xz, xn, hr, hz, hn, hprev[b * hp_rs + ih]);
        hs[b * hs_rs + ih] = f.h;
        if (hnext) hnext[b * hn_rs + ih] = f.h;
        if (gates) {
            float* gp = gates + b * g_rs + (int64_t)i * 4 * H + c0 + cc;
            gp[0] = f.r;
            gp[H] = f.z;
            gp[2 * H] = f.n;
            gp[3 * H] = hn;
        }
    }
}

// Gate backward of step t, one thread per (row, node, feature): dh = dhs[:, t] + the carry from
// step t + 1 (null at the last step); writes dP[:, t] = [pr | pz | pn | pn r] and dhz = dh z.
__global__ __launch_bounds__(256) void k_gru_gate_bwd(const float* __restrict__ dhs, const float* __restrict__ dhc,
                                                      const float* __restrict__ gates, const float* __restrict__ hprev,
                                                      float* __restrict__ dP, float* __restrict__ dhz, int64_t B, int T,
                                                      int t, int J, int H) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t JH = (int64_t)J * H;
    if (e >= B * JH) return;
    const int64_t b = e / JH;
    const int ih = (int)(e % JH);
    const int i = ih / H, cc = ih % H;
    const int64_t o1 = gru::at4(b, t, i, T, J, H) + cc, o4 = gru::at4(b, t, i, T, J, 4 * H) + cc;
    const float dh = dhs[o1] + (dhc ? dhc[e] : 0.f);
    const gru::GateBwd<float> g =
        gru::gate_backward(dh, gates[o4], gates[o4 + H], gates[o4 + 2 * H], gates[o4 + 3 * H], hprev[o1]);
    dP[o4] = g.pr;
    dP[o4 + H] = g.pz;
    dP[o4 + 2 * H] = g.pn;
    dP[o4 + 3 * H] = g.pnr;
    dhz[e] = g.carry;
}

// Node j = blockIdx.x, kGruRT rows from blockIdx.y * kGruRT, step t:
//   dc[b, t, j, :] = sum_i gx_t[i, j] dHh[b, t, i, :]     (kept in LDS and written for the batched dW)
//   dh_prev[b, j, :] = dhz[b, j, :] + W_hh[type j]^T dc[b, t, j, :]
// The W^T product: `groups` = 256 / H thread groups split the 3H reduction, thread -> (group,
// feature k) with W unit-stride over k; the groups' partials are summed in group order.
__global__ __launch_bounds__(256) void k_gru_bwd_hh(const float* __restrict__ dP, const float* __restrict__ gx,
                                                    const float* __restrict__ W, NodeTypes nt,
                                                    const float* __restrict__ dhz, float* __restrict__ dc,
                                                    float* __restrict__ dhc, int64_t B, int T, int t, int J, int H) {
    __shared__ __attribute__((aligned(16))) float sdc[kGruRT][3 * kGruMaxH];
    __shared__ float spart[kGruRT * 256];
    __shared__ float sgc[kMaxNodes];
    const int j = blockIdx.x, H3 = 3 * H, tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.y * kGruRT;
    if (tid < J) sgc[tid] = gx[tid * J + j];
    __syncthreads();
    for (int e = tid; e < kGruRT * H3; e += 256) {
        const int r = e / H3, n = e - r * H3;
        float acc = 0.f;
        if (b0 + r < B) {
            const float* p = dP + gru::at4(b0 + r, t, 0, T, J, 4 * H) + gru::hh_col(n, H);
            for (int i = 0; i < J; ++i) acc = fmaf(sgc[i], p[(int64_t)i * 4 * H], acc);
            dc[gru::at4(b0 + r, t, j, T, J, H3) + n] = acc;
        }
        sdc[r][n] = acc;
    }
    __syncthreads();
    const int groups = 256 / H;  // >= 1 (H <= kGruMaxH)
    const int nper = ((H3 + groups - 1) / groups + 3) & ~3;
    const int g = tid / H, k = tid - g * H;
    if (g < groups) {
        float acc[kGruRT];
#pragma unroll
        for (int r = 0; r < kGruRT; ++r) acc[r] = 0.f;
        const float* Wj = W + (int64_t)nt.t[j] * H3 * H;
        const int n1 = min(H3, (g + 1) * nper);
        for (int n = g * nper; n < n1; n += 4) {  // H3 % 4 == 0: whole groups of 4
            const float w0 = Wj[(int64_t)n * H + k], w1 = Wj[(int64_t)(n + 1) * H + k];
            const float w2 = Wj[(int64_t)(n + 2) * H + k], w3 = Wj[(int64_t)(n + 3) * H + k];
#pragma unroll
            for (int r = 0; r < kGruRT; ++r) {
                const float4 d = *reinterpret_cast<const float4*>(&sdc[r][n]);
                acc[r] = fmaf(w0, d.x, acc[r]);
                acc[r] = fmaf(w1, d.y, acc[r]);
                acc[r] = fmaf(w2, d.z, acc[r]);
                acc[r] = fmaf(w3, d.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kGruRT; ++r) spart[(g * kGruRT + r) * H + k] = acc[r];
    }
    __syncthreads();
    for (int e = tid; e < kGruRT * H; e += 256) {
        const int r = e / H, kk = e - r * H;
        if (b0 + r >= B) continue;
        const int64_t o = (b0 + r) * (int64_t)J * H + (int64_t)j * H + kk;
        float acc = dhz[o];
        for (int gg = 0; gg < groups; ++gg) acc += spart[(gg * kGruRT + r) * H + kk];
        dhc[o] = acc;
    }
}

// da[b, ta, j, n] = sum over the steps t of slab ta (one step when Ta = T, all T in order when
// Ta = 1) of sum_i gx_t[i, j] dX[b, t, i, n].  Workgroup per (b, ta) and 64 columns; thread ->
// (column, nodes j = q, q + 4, ...).
__global__ __launch_bounds__(256) void k_gru_da(const float* __restrict__ dP, const float* __restrict__ gx, int Tg,
                                                float* __restrict__ da, int Ta, int T, int J, int H) {
    __shared__ float sx[kMaxNodes][64];
    __shared__ float sg[kMaxNodes][kMaxNodes + 1];
    const int64_t b = blockIdx.x / Ta;
    const int ta = blockIdx.x % Ta, n0 = blockIdx.y * 64, H3 = 3 * H;
    const int cc = threadIdx.x & 63, q = threadIdx.x >> 6;
    float acc[kMaxNodes / 4];
#pragma unroll
    for (int u = 0; u < kMaxNodes / 4; ++u) acc[u] = 0.f;
    const int t0 = Ta == 1 ? 0 : ta, t1 = Ta == 1 ? T : ta + 1;
    for (int t = t0; t < t1; ++t) {
        __syncthreads();
        for (int e = threadIdx.x; e < J * 64; e += 256) {
            const int i = e >> 6, c = e & 63;
            sx[i][c] = n0 + c < H3 ? dP[gru::at4(b, t, i, T, J, 4 * H) + n0 + c] : 0.f;
        }
        if (t == t0 || Tg != 1) {
            const float* g = gx + gru::step_of(t, Tg) * J * J;
            for (int e = threadIdx.x; e < J * J; e += 256) sg[e / J][e % J] = g[e];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kMaxNodes / 4; ++u) {
            const int j = q + 4 * u;
            if (j < J) {
                float s = acc[u];
                for (int i = 0; i < J; ++i) s = fmaf(sg[i][j], sx[i][cc], s);
                acc[u] = s;
            }
        }
    }
    if (n0 + cc >= H3) return;
#pragma unroll
    for (int u = 0; u < kMaxNodes / 4; ++u) {
        const int j = q + 4 * u;
        if (j < J) da[gru::at4(b, ta, j, Ta, J, H3) + n0 + cc] = acc[u];
    }
}

// part[t][chunk] (J, J) = sum over the chunk's rows b of dX[b, t] a[b, t]^T + dHh[b, t] c[b, t]^T
// (contraction over the 3H columns, 32 at a time through LDS).  Thread (ty, tx) owns the outputs
// (ty + 16 p, tx + 16 q), p, q < TI (J <= 16 TI).
template <int TI>
__global__ __launch_bounds__(256) void k_gru_dgx_part(const float* __restrict__ dP, const float* __restrict__ a, int Ta,
                                                      const float* __restrict__ c, float* __restrict__ part, int64_t B,
                                                      int T, int J, int H) {
    __shared__ float sd[16 * TI][33];
    __shared__ float sv[16 * TI][33];
    const int t = blockIdx.x, chunk = blockIdx.y, chunks = gridDim.y, H3 = 3 * H;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    float acc[TI][TI];
#pragma unroll
    for (int p = 0; p < TI; ++p)
#pragma unroll
        for (int q = 0; q < TI; ++q) acc[p][q] = 0.f;
    const int64_t b0 = (int64_t)chunk * kGruDgxRows, b1 = min(B, b0 + kGruDgxRows);
    for (int64_t b = b0; b < b1; ++b) {
        for (int pass = 0; pass < 2; ++pass) {
            const float* V = pass == 0 ? a + gru::at4(b, gru::step_of(t, Ta), 0, Ta, J, H3) : c + gru::at4(b, t, 0, T, J, H3);
            const float* D = dP + gru::at4(b, t, 0, T, J, 4 * H);
            for (int n0 = 0; n0 < H3; n0 += 32) {
                __syncthreads();
                for (int e = threadIdx.x; e < 16 * TI * 32; e += 256) {
                    const int i = e >> 5, q = e & 31, n = n0 + q;
                    const bool ok = i < J && n < H3;
                    sd[i][q] = ok ? D[(int64_t)i * 4 * H + (pass ? gru::hh_col(n, H) : n)] : 0.f;
                    sv[i][q] = ok ? V[(int64_t)i * H3 + n] : 0.f;
                }
                __syncthreads();
#pragma unroll 8
                for (int q = 0; q < 32; ++q) {
                    float dv[TI], vv[TI];
#pragma unroll
                    for (int p = 0; p < TI; ++p) {
                        dv[p] = sd[ty + 16 * p][q];
                        vv[p] = sv[tx + 16 * p][q];
                    }
#pragma unroll
                    for (int p = 0; p < TI; ++p)
#pragma unroll
                        for (int r = 0; r < TI; ++r) acc[p][r] = fmaf(dv[p], vv[r], acc[p][r]);
                }
            }
        }
    }
    float* out = part + ((int64_t)t * chunks + chunk) * J * J;
#pragma unroll
    for (int p = 0; p < TI; ++p)
#pragma unroll
        for (int q = 0; q < TI; ++q) {
            const int i = ty + 16 * p, j = tx + 16 * q;
            if (i < J && j < J) out[i * J + j] = acc[p][q];
        }
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// gx table: one wave per row i (rows are independent under the row-L1 normalise), lane j, the
// steps in sequence inside the kernel.  out (T, J, J).
__global__ __launch_bounds__(64) void k_gxt_fwd(const float* __restrict__ G, const float* __restrict__ Gadd, int J,
                                                int T, int normalize0, float eps, float* __restrict__ out) {
    const int i = blockIdx.x, j = threadIdx.x;
    const bool ok = j < J;
    float v = ok ? G[i * J + j] : 0.f;
    const float add = (ok && Gadd) ? Gadd[i * J + j] : 0.f;
    if (normalize0) v = v / gru::l1_den(wave_sum64(fabsf(v)), eps);
    for (int t = 0; t < T; ++t) {
        if (ok) out[((int64_t)t * J + i) * J + j] = v;
        const float u = v + add;
        v = u / gru::l1_den(wave_sum64(fabsf(u)), eps);
    }
}

// backward of the table from dgxt (T, J, J), with the forward's output gxt: dG, dGadd (nullable)
__global__ __launch_bounds__(64) void k_gxt_bwd(const float* __restrict__ G, const float* __restrict__ Gadd,
                                                const float* __restrict__ gxt, const float* __restrict__ dgxt, int J,
                                                int T, int normalize0, float eps, float* __restrict__ dG,
                                                float* __restrict__ dGadd) {
    const int i = blockIdx.x, j = threadIdx.x;
    const bool ok = j < J;
    const float add = (ok && Gadd) ? Gadd[i * J + j] : 0.f;
    float g = ok ? dgxt[((int64_t)(T - 1) * J + i) * J + j] : 0.f;
    float dadd = 0.f;
    for (int t = T - 2; t >= 0; --t) {
        const int64_t o = ((int64_t)t * J + i) * J + j;
        const float u = ok ? gxt[o] + add : 0.f;
        const float nrm = wave_sum64(fabsf(u)), dot = wave_sum64(g * u);
        const float du = gru::l1_backward(g, u, dot, nrm, eps);
        dadd += du;
        g = (ok ? dgxt[o] : 0.f) + du;
    }
    if (normalize0) {
        const float u = ok ? G[i * J + j] : 0.f;
        const float nrm = wave_sum64(fabsf(u)), dot = wave_sum64(g * u);
        g = gru::l1_backward(g, u, dot, nrm, eps);
    }
    if (ok) {
        dG[i * J + j] = g;
        if (dGadd) dGadd[i * J + j] = dadd;
    }
}

size_t al256(size_t nfloat) { return (nfloat * sizeof(float) + 255) & ~(size_t)255; }

// workspace layout (forward and backward share one size)
struct GruWS {
    float *wt, *ctmp;                                // forward
    float *dP, *dc, *dhz, *dhc, *ident, *part, *gl;  // backward
    int64_t* types;
    size_t gl_bytes;
};

size_t gru_carve(int64_t B, int T, int J, int H, int n_types, char* base, GruWS* w) {
    const int types = n_types > 0 ? n_types : 1;
    const size_t BJ = (size_t)B * J;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    GruWS t{};
    GruWS& o = w ? *w : t;
    // forward
    o.wt = (float*)take((size_t)types * 3 * H * H * sizeof(float));
    o.ctmp = (float*)take(BJ * 3 * H * sizeof(float));
    const size_t fwd = off;
    // backward (over the same bytes)
    off = 0;
    o.dP = (float*)take(BJ * T * 4 * H * sizeof(float));
    o.dc = (float*)take(BJ * T * 3 * H * sizeof(float));
    o.dhz = (float*)take(BJ * H * sizeof(float));
    o.dhc = (float*)take(BJ * H * sizeof(float));
    o.ident = (float*)take((size_t)J * J * sizeof(float));
    o.types = (int64_t*)take((size_t)kMaxNodes * sizeof(int64_t));
    const size_t chunks = (size_t)((B + kGruDgxRows - 1) / kGruDgxRows);
    o.part = (float*)take((size_t)T * chunks * J * J * sizeof(float));
    o.gl_bytes = sd_gl_train_workspace_bytes(B * T, J, H, 3 * H, n_types);
    o.gl = (float*)take(o.gl_bytes);
    return off > fwd ? off : fwd;
}

}  // namespace
}  // namespace sd

extern "C" {

size_t sd_gru_train_workspace_bytes(int64_t rows, int32_t T, int32_t J, int32_t H, int32_t n_types) {
    if (rows < 0 || T < 1 || J < 1 || J > sd::kMaxNodes || H < 1 || n_types < 0) return 0;
    return sd::gru_carve(rows, T, J, H, n_types, nullptr, nullptr);
}

int sd_gru_train_forward(const float* a, int32_t Ta, const float* h0, const float* gx, int32_t Tg, const float* W_hh,
                         const float* b_hh, const int64_t* node_types, int32_t n_types, int64_t rows, int32_t T,
                         int32_t J, int32_t H, float* hs, float* hprev, float* c, float* gates, void* workspace,
                         size_t workspace_bytes, void* stream) {
    sd::NodeTypes nt;
    if (int rc = sd::seq_check("sd_gru_train_forward", rows, T, Ta, Tg, J, H, node_types, n_types, false, &nt)) return rc;
    const bool keep = hprev || c || gates;
    if (keep && !(hprev && c && gates))
        return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: hprev, c and gates are kept together (all or none)");
    if (rows == 0) return SD_OK;
    if (!a) return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: a is null");
    if (!h0) return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: h0 is null");
    if (!gx) return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: gx is null");
    if (!W_hh) return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: W_hh is null");
    if (!hs) return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: hs is null");
    if (!workspace || workspace_bytes < sd_gru_train_workspace_bytes(rows, T, J, H, n_types))
        return sd::set_error(SD_E_INVALID, "sd_gru_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    sd::GruWS w;
    sd::gru_carve(rows, T, J, H, n_types, (char*)workspace, &w);
    const int types = n_types > 0 ? n_types : 1;
    const int H3 = 3 * H;
    const int64_t JH = (int64_t)J * H, JH3 = (int64_t)J * H3;
    const int64_t nw = (int64_t)types * H3 * H;
    hipLaunchKernelGGL(sd::k_gru_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, W_hh, (int64_t)types, H,
                       w.wt);
    SD_HIP(hipGetLastError());
    if (keep) {
        hipLaunchKernelGGL(sd::k_gru_copy_rows, dim3((unsigned)((rows * JH + 255) / 256)), dim3(256), 0, s, h0, JH, hprev,
                           (int64_t)T * JH, rows, (int)JH);
        SD_HIP(hipGetLastError());
    }
    const int hh_threads = ((H3 < 1024 ? H3 : 1024) + 63) & ~63;
    const dim3 hh_grid((unsigned)J, (unsigned)((rows + sd::kGruRT - 1) / sd::kGruRT));
    const dim3 gate_grid((unsigned)rows, (unsigned)(H / sd::kGruCH));
    for (int t = 0; t < T; ++t) {
        const float* hp = t == 0 ? h0 : hs + (int64_t)(t - 1) * JH;
        const int64_t hp_rs = t == 0 ? JH : (int64_t)T * JH;
        float* ct = keep ? c + (int64_t)t * JH3 : w.ctmp;
        const int64_t c_rs = keep ? (int64_t)T * JH3 : JH3;
        hipLaunchKernelGGL(sd::k_gru_hh, hh_grid, dim3(hh_threads), 0, s, hp, hp_rs, w.wt, b_hh, nt, ct, c_rs, rows, J, H);
        SD_HIP(hipGetLastError());
        const float* at = a + (int64_t)sd::gru::step_of(t, Ta) * JH3;
        float* hn = (keep && t + 1 < T) ? hprev + (int64_t)(t + 1) * JH : nullptr;
        hipLaunchKernelGGL(sd::k_gru_gate, gate_grid, dim3(256), 0, s, at, (int64_t)Ta * JH3, ct, c_rs,
                           gx + sd::gru::step_of(t, Tg) * J * J, hp, hp_rs, hs + (int64_t)t * JH, (int64_t)T * JH, hn,
                           (int64_t)T * JH, keep ? gates + (int64_t)t * J * 4 * H : nullptr, (int64_t)T * J * 4 * H, J, H);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

int sd_gru_train_backward(const float* dhs, const float* a, int32_t Ta, const float* gx, int32_t Tg, const float* W_hh,
                          const int64_t* node_types, int32_t n_types, const float* hprev, const float* c,
                          const float* gates, int64_t rows, int32_t T, int32_t J, int32_t H, float* da, float* dh0,
                          float* dgx, float* dW_hh, float* db_hh, void* workspace, size_t workspace_bytes, void* stream) {
    sd::NodeTypes nt;
    if (int rc = sd::seq_check("sd_gru_train_backward", rows, T, Ta, Tg, J, H, node_types, n_types, dgx != nullptr, &nt)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int types = n_types > 0 ? n_types : 1;
    const int H3 = 3 * H;
    if (rows == 0) {  // empty batch: zero parameter gradients
        if (dgx) SD_HIP(hipMemsetAsync(dgx, 0, (size_t)Tg * J * J * sizeof(float), s));
        if (dW_hh) SD_HIP(hipMemsetAsync(dW_hh, 0, (size_t)types * H3 * H * sizeof(float), s));
        if (db_hh) SD_HIP(hipMemsetAsync(db_hh, 0, (size_t)types * H3 * sizeof(float), s));
        return SD_OK;
    }
    if (!dhs) return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: dhs is null");
    if (!a) return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: a is null");
    if (!gx) return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: gx is null");
    if (!W_hh) return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: W_hh is null");
    if (!hprev || !c || !gates)
        return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: the forward's state (hprev, c, gates) is null");
    if (!workspace || workspace_bytes < sd_gru_train_workspace_bytes(rows, T, J, H, n_types))
        return sd::set_error(SD_E_INVALID, "sd_gru_train_backward: workspace too small");
    sd::GruWS w;
    sd::gru_carve(rows, T, J, H, n_types, (char*)workspace, &w);
    const int64_t JH = (int64_t)J * H;
    const dim3 hh_grid((unsigned)J, (unsigned)((rows + sd::kGruRT - 1) / sd::kGruRT));
    const unsigned ew_blocks = (unsigned)((rows * JH + 255) / 256);
    // reverse sweep
    for (int t = T - 1; t >= 0; --t) {
        hipLaunchKernelGGL(sd::k_gru_gate_bwd, dim3(ew_blocks), dim3(256), 0, s, dhs, t == T - 1 ? nullptr : w.dhc, gates,
                           hprev, w.dP, w.dhz, rows, T, t, J, H);
        SD_HIP(hipGetLastError());
        hipLaunchKernelGGL(sd::k_gru_bwd_hh, hh_grid, dim3(256), 0, s, w.dP, gx + sd::gru::step_of(t, Tg) * J * J, W_hh,
                           nt, w.dhz, w.dc, w.dhc, rows, T, t, J, H);
        SD_HIP(hipGetLastError());
    }
    if (dh0) SD_HIP(hipMemcpyAsync(dh0, w.dhc, (size_t)rows * JH * sizeof(float), hipMemcpyDeviceToDevice, s));
    // batched over all rows x steps
    if (da) {
        hipLaunchKernelGGL(sd::k_gru_da, dim3((unsigned)(rows * Ta), (unsigned)((H3 + 63) / 64)), dim3(256), 0, s, w.dP,
                           gx, Tg, da, Ta, T, J, H);
        SD_HIP(hipGetLastError());
    }
    if (dgx) {
        const int chunks = (int)((rows + sd::kGruDgxRows - 1) / sd::kGruDgxRows);
        const dim3 grid((unsigned)T, (unsigned)chunks);
        if (J <= 16)
            hipLaunchKernelGGL(sd::k_gru_dgx_part<1>, grid, dim3(256), 0, s, w.dP, a, Ta, c, w.part, rows, T, J, H);
        else if (J <= 32)
            hipLaunchKernelGGL(sd::k_gru_dgx_part<2>, grid, dim3(256), 0, s, w.dP, a, Ta, c, w.part, rows, T, J, H);
        else
            hipLaunchKernelGGL(sd::k_gru_dgx_part<4>, grid, dim3(256), 0, s, w.dP, a, Ta, c, w.part, rows, T, J, H);
        SD_HIP(hipGetLastError());
        const int cnt = (Tg == 1 ? T : 1) * chunks;
        const int64_t total = (int64_t)Tg * J * J;
        hipLaunchKernelGGL(sd::k_seq_dgx_sum, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, w.part, cnt, J * J, total,
                           dgx);
        SD_HIP(hipGetLastError());
    }
    if (dW_hh || db_hh) {
        // dW_hh = sum_{b,t} dc (x) h_{t-1}, db_hh = sum_{b,t} dc: the graph-linear's weight / bias
        // gradient over B T rows with an identity mixing matrix (one pass, fixed order)
        hipLaunchKernelGGL(sd::k_seq_identity, dim3((unsigned)((J * J + 255) / 256)), dim3(256), 0, s, w.ident, J);
        SD_HIP(hipGetLastError());
        if (n_types > 0) {
            hipLaunchKernelGGL(sd::k_seq_write_types, dim3(1), dim3(64), 0, s, nt, J, w.types);
            SD_HIP(hipGetLastError());
        }
        // (z feeds only dghat, which is not asked for; the entry still wants a non-null pointer)
        const int rc = sd_gl_train_backward(hprev, c, w.dc, W_hh, n_types > 0 ? w.types : nullptr, n_types, w.ident,
                                            rows * T, J, H, H3, nullptr, dW_hh, db_hh, nullptr, w.gl, w.gl_bytes, stream);
        if (rc != SD_OK) return rc;
    }
    return SD_OK;
}

int sd_gx_table_forward(const float* G, const float* G_add, int32_t J, int32_t T, int32_t normalize0, float eps,
                        float* gxt, void* stream) {
    if (J < 1 || J > sd::kMaxNodes) return sd::set_error(SD_E_INVALID, "sd_gx_table_forward: J outside 1..64");
    if (T < 1) return sd::set_error(SD_E_INVALID, "sd_gx_table_forward: T must be >= 1");
    if (!G) return sd::set_error(SD_E_INVALID, "sd_gx_table_forward: G is null");
    if (!gxt) return sd::set_error(SD_E_INVALID, "sd_gx_table_forward: gxt is null");
    hipLaunchKernelGGL(sd::k_gxt_fwd, dim3((unsigned)J), dim3(64), 0, (hipStream_t)stream, G, G_add, J, T, normalize0, eps,
                       gxt);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

int sd_gx_table_backward(const float* G, const float* G_add, const float* gxt, const float* dgxt, int32_t J, int32_t T,
                         int32_t normalize0, float eps, float* dG, float* dG_add, void* stream) {
    if (J < 1 || J > sd::kMaxNodes) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: J outside 1..64");
    if (T < 1) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: T must be >= 1");
    if (!G) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: G is null");
    if (!gxt) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: gxt is null");
    if (!dgxt) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: dgxt is null");
    if (!dG) return sd::set_error(SD_E_INVALID, "sd_gx_table_backward: dG is null");
    hipLaunchKernelGGL(sd::k_gxt_bwd, dim3((unsigned)J), dim3(64), 0, (hipStream_t)stream, G, G_add, gxt, dgxt, J, T,
                       normalize0, eps, dG, dG_add);
    SD_HIP(hipGetLastError());
    return SD_OK;
}

}  // extern "C"
