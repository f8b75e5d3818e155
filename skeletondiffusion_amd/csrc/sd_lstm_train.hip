// Training side of the graph-LSTM: the recurrent core of StaticGraphLSTMCell
// (src/core/network/layers/recurrent.py:126-167, clockwork off) over a whole sequence with the
// state backward needs, and its backward through time.  Per batch row and step t:
//   P_t = a_t + W_hh[type j] h_{t-1} + b_hh[type j]                 (J, 4H), unmixed; a_t = W_ih x_t
//   Q_t = gx_t P_t                                                   one mixing, of the sum
//   i, f, o = sigma(Q_i, Q_f, Q_o), g = tanh(Q_g),  s_t = f s_{t-1} + i g,  h_t = o tanh(s_t)
// Launch structure (that of sd_gru_train.hip):
//   forward, per step:  k_lstm_hh (P_t, one workgroup per (node, 8 rows)), k_lstm_gate (mix + gates)
//   backward, per step: k_lstm_gate_bwd (dQ_t, the cell-state carry ds f),
//                       k_lstm_bwd_hh (dP_t = gx_t^T dQ_t, dh_{t-1} = W_hh^T dP_t)
//   after the reverse sweep, over all B T rows at once: da = dP (summed over the steps in order
//   when Ta = 1), dW_hh / db_hh (the per-type GEMM and bias reduction of sd_gl_train_backward on
//   x = h_{t-1}, dy = dP with an identity mixing matrix), dgx = sum_b dQ P^T (k_lstm_dgx_part +
//   k_seq_dgx_sum).
// Saved state per (row, step, node): P_t (4H), the gate record [i | f | g | o] (4H) and s_t (H);
// h_{t-1} is read from h0 / hs.  Every reduction over rows and steps runs in a fixed order (no float
// atomics): two runs give the same bits.  The gate math is sd_lstm_gates.h, shared with the host
// emulation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_internal.h"
#include "sd_lstm_gates.h"

namespace sd {
namespace {

#include "sd_seq_train.h"

constexpr int kLstmMaxH = kSeqMaxH;        // hidden width the per-step kernels' LDS tiles are sized for
constexpr int kLstmRT = kSeqRT;            // rows per workgroup of k_lstm_hh / k_lstm_bwd_hh
constexpr int kLstmCH = 16;                // hidden features per workgroup of k_lstm_gate (H % 16 == 0)
constexpr int kLstmDgxRows = kSeqDgxRows;  // rows per partial of the dgx reduction

// W (types, 4H, H) -> Wt (types, H, 4H): k_lstm_hh reads unit-stride over the output column
__global__ void k_lstm_transpose_w(const float* __restrict__ W, int64_t types, int H, float* __restrict__ Wt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int H4 = 4 * H;
    if (e >= types * H4 * H) return;
    const int64_t t = e / ((int64_t)H4 * H);
    const int rem = (int)(e % ((int64_t)H4 * H));
    const int k = rem / H4, n = rem % H4;
    Wt[e] = W[(t * H4 + n) * H + k];
}

// hp (B, T, J, H): hp[b, 0] = h0[b], hp[b, t] = hs[b, t - 1] (the x operand of the batched dW_hh)
__global__ void k_lstm_hprev(const float* __restrict__ h0, const float* __restrict__ hs, float* __restrict__ hp,
                             int64_t B, int T, int64_t JH) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * T * JH) return;
    const int64_t bt = e / JH, k = e % JH;
    const int64_t b = bt / T;
    const int t = (int)(bt % T);
    hp[e] = t == 0 ? h0[b * JH + k] : hs[e - JH];
}

// P[b, j, :] = a[b, j, :] + W_hh[type j] h[b, j, :] + b_hh[type j] for node j = blockIdx.x and the
// kLstmRT rows from blockIdx.y * kLstmRT: the rows' h in LDS (16-B broadcast reads), thread ->
// output column n, Wt unit-stride over n.  a / h / P rows at strides a_rs / h_rs / p_rs.
__global__ __launch_bounds__(1024) void k_lstm_hh(const float* __restrict__ a, int64_t a_rs, const float* __restrict__ h,
                                                  int64_t h_rs, const float* __restrict__ Wt,
                                                  const float* __restrict__ bias, NodeTypes nt, float* __restrict__ P,
                                                  int64_t p_rs, int64_t B, int J, int H) {
    __shared__ __attribute__((aligned(16))) float sh[kLstmRT][kLstmMaxH];
    const int j = blockIdx.x, H4 = 4 * H;
    const int64_t b0 = (int64_t)blockIdx.y * kLstmRT;
    const int t = nt.t[j];
    for (int e = threadIdx.x; e < kLstmRT * H; e += blockDim.x) {
        const int r = e / H, k = e - r * H;
        sh[r][k] = b0 + r < B ? h[(b0 + r) * h_rs + (int64_t)j * H + k] : 0.f;
    }
    __syncthreads();
    const float* W = Wt + (int64_t)t * H * H4;
    for (int n = threadIdx.x; n < H4; n += blockDim.x) {
        float acc[kLstmRT];
        const float bv = bias ? bias[(int64_t)t * H4 + n] : 0.f;
#pragma unroll
        for (int r = 0; r < kLstmRT; ++r) acc[r] = bv;
        for (int k = 0; k < H; k += 4) {
            const float w0 = W[(int64_t)k * H4 + n], w1 = W[(int64_t)(k + 1) * H4 + n];
            const float w2 = W[(int64_t)(k + 2) * H4 + n], w3 = W[(int64_t)(k + 3) * H4 + n];
#pragma unroll
            for (int r = 0; r < kLstmRT; ++r) {
                const float4 hv = *reinterpret_cast<const float4*>(&sh[r][k]);
                acc[r] = fmaf(w0, hv.x, acc[r]);
                acc[r] = fmaf(w1, hv.y, acc[r]);
                acc[r] = fmaf(w2, hv.z, acc[r]);
                acc[r] = fmaf(w3, hv.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kLstmRT; ++r)
            if (b0 + r < B) {
                const int64_t o = (int64_t)j * H4 + n;
                P[(b0 + r) * p_rs + o] = a[(b0 + r) * a_rs + o] + acc[r];
            }
    }
}

// One workgroup per (row b, kLstmCH hidden features): the four gate column groups of P_t[b] for
// those features and gx_t in LDS; thread -> (node i, feature) mixes over the nodes and applies the
// gates.  Writes h_t to hs, s_t to sout (and sout2 when given) and the gate record when state is kept.
__global__ __launch_bounds__(256) void k_lstm_gate(const float* __restrict__ P, int64_t p_rs, const float* __restrict__ gx,
                                                   const float* __restrict__ sprev, int64_t sp_rs, float* __restrict__ hs,
                                                   int64_t hs_rs, float* __restrict__ sout, int64_t so_rs,
                                                   float* __restrict__ sout2, int64_t so2_rs, float* __restrict__ gates,
                                                   int64_t g_rs, int J, int H) {
    __shared__ float sp[kMaxNodes][4 * kLstmCH];
    __shared__ float sg[kMaxNodes][kMaxNodes + 1];
    const int64_t b = blockIdx.x;
    const int c0 = blockIdx.y * kLstmCH, H4 = 4 * H;
    for (int e = threadIdx.x; e < J * 4 * kLstmCH; e += 256) {
        const int j = e / (4 * kLstmCH), q = e - j * 4 * kLstmCH;
        const int col = (q / kLstmCH) * H + c0 + (q % kLstmCH);
        sp[j][q] = P[b * p_rs + (int64_t)j * H4 + col];
    }
    for (int e = threadIdx.x; e < J * J; e += 256) sg[e / J][e % J] = gx[e];
    __syncthreads();
    for (int o = threadIdx.x; o < J * kLstmCH; o += 256) {
        const int i = o / kLstmCH, cc = o % kLstmCH;
        float qi = 0.f, qf = 0.f, qg = 0.f, qo = 0.f;
        for (int j = 0; j < J; ++j) {
            const float g = sg[i][j];
            qi = fmaf(g, sp[j][cc], qi);
            qf = fmaf(g, sp[j][kLstmCH + cc], qf);
            qg = fmaf(g, sp[j][2 * kLstmCH + cc], qg);
            qo = fmaf(g, sp[j][3 * kLstmCH + cc], qo);
        }
        const int64_t ih = (int64_t)i * H + c0 + cc;
        const lstm::GateFwd<float> f = lstm::gate_forward(qi, qf, qg, qo, sprev[b * sp_rs + ih]);
        hs[b * hs_rs + ih] = f.h;
        sout[b * so_rs + ih] = f.s;
        if (sout2) sout2[b * so2_rs + ih] = f.s;
        if (gates) {
            float* gp = gates + b * g_rs + (int64_t)i * H4 + c0 + cc;
            gp[0] = f.i;
            gp[H] = f.f;
            gp[2 * H] = f.g;
            gp[3 * H] = f.o;
        }
    }
}

// Gate backward of step t, one thread per (row, node, feature): dh = dhs[:, t] + the carry from
// step t + 1, ds likewise (both null at the last step); writes dQ[:, t] and the cell carry ds f.
__global__ __launch_bounds__(256) void k_lstm_gate_bwd(const float* __restrict__ dhs, const float* __restrict__ dhc,
                                                       const float* __restrict__ gates, const float* __restrict__ sseq,
                                                       const float* __restrict__ s0, float* __restrict__ dQ,
                                                       float* __restrict__ cs, int first, int64_t B, int T, int t, int J,
                                                       int H) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t JH = (int64_t)J * H;
    if (e >= B * JH) return;
    const int64_t b = e / JH;
    const int ih = (int)(e % JH);
    const int i = ih / H, cc = ih % H;
    const int64_t o1 = lstm::at4(b, t, i, T, J, H) + cc, o4 = lstm::at4(b, t, i, T, J, 4 * H) + cc;
    const float dh = dhs[o1] + (first ? 0.f : dhc[e]);
    const float sprev = t == 0 ? s0[e] : sseq[o1 - JH];
    const lstm::GateBwd<float> g = lstm::gate_backward(dh, first ? 0.f : cs[e], gates[o4], gates[o4 + H],
                                                       gates[o4 + 2 * H], gates[o4 + 3 * H], sseq[o1], sprev);
    dQ[o4] = g.qi;
    dQ[o4 + H] = g.qf;
    dQ[o4 + 2 * H] = g.qg;
    dQ[o4 + 3 * H] = g.qo;
    cs[e] = g.carry;
}

// Node j = blockIdx.x, kLstmRT rows from blockIdx.y * kLstmRT, step t:
//   dP[b, t, j, :] = sum_i gx_t[i, j] dQ[b, t, i, :]       (kept in LDS and written for the batched part)
//   dh_prev[b, j, :] = W_hh[type j]^T dP[b, t, j, :]
// The W^T product: `groups` = 256 / H thread groups split the 4H reduction, thread -> (group,
// feature k) with W unit-stride over k; the groups' partials are summed in group order.
__global__ __launch_bounds__(256) void k_lstm_bwd_hh(const float* __restrict__ dQ, const float* __restrict__ gx,
                                                     const float* __restrict__ W, NodeTypes nt, float* __restrict__ dP,
                                                     float* __restrict__ dhc, int64_t B, int T, int t, int J, int H) {
    __shared__ __attribute__((aligned(16))) float sdp[kLstmRT][4 * kLstmMaxH];
    __shared__ float spart[kLstmRT * 256];
    __shared__ float sgc[kMaxNodes];
    const int j = blockIdx.x, H4 = 4 * H, tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.y * kLstmRT;
    if (tid < J) sgc[tid] = gx[tid * J + j];
    __syncthreads();
    for (int e = tid; e < kLstmRT * H4; e += 256) {
        const int r = e / H4, n = e - r * H4;
        float acc = 0.f;
        if (b0 + r < B) {
            const float* p = dQ + lstm::at4(b0 + r, t, 0, T, J, H4) + n;
            for (int i = 0; i < J; ++i) acc = fmaf(sgc[i], p[(int64_t)i * H4], acc);
            dP[lstm::at4(b0 + r, t, j, T, J, H4) + n] = acc;
        }
        sdp[r][n] = acc;
    }
    __syncthreads();
    const int groups = 256 / H;  // >= 1 (H <= kLstmMaxH)
    const int nper = ((H4 + groups - 1) / groups + 3) & ~3;
    const int g = tid / H, k = tid - g * H;
    if (g < groups) {
        float acc[kLstmRT];
#pragma unroll
        for (int r = 0; r < kLstmRT; ++r) acc[r] = 0.f;
        const float* Wj = W + (int64_t)nt.t[j] * H4 * H;
        const int n1 = min(H4, (g + 1) * nper);
        for (int n = g * nper; n < n1; n += 4) {  // H4 % 4 == 0: whole groups of 4
            const float w0 = Wj[(int64_t)n * H + k], w1 = Wj[(int64_t)(n + 1) * H + k];
            const float w2 = Wj[(int64_t)(n + 2) * H + k], w3 = Wj[(int64_t)(n + 3) * H + k];
#pragma unroll
            for (int r = 0; r < kLstmRT; ++r) {
                const float4 d = *reinterpret_cast<const float4*>(&sdp[r][n]);
                acc[r] = fmaf(w0, d.x, acc[r]);
                acc[r] = fmaf(w1, d.y, acc[r]);
                acc[r] = fmaf(w2, d.z, acc[r]);
                acc[r] = fmaf(w3, d.w, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kLstmRT; ++r) spart[(g * kLstmRT + r) * H + k] = acc[r];
    }
    __syncthreads();
    for (int e = tid; e < kLstmRT * H; e += 256) {
        const int r = e / H, kk = e - r * H;
        if (b0 + r >= B) continue;
        float acc = 0.f;
        for (int gg = 0; gg < groups; ++gg) acc += spart[(gg * kLstmRT + r) * H + kk];
        dhc[(b0 + r) * (int64_t)J * H + (int64_t)j * H + kk] = acc;
    }
}

// da (B, Ta, J, 4H) from dP (B, T, J, 4H): a copy when Ta = T, the sum over the steps in order
// when Ta = 1.  n = J 4H elements per (row, step).
__global__ __launch_bounds__(256) void k_lstm_da(const float* __restrict__ dP, float* __restrict__ da, int64_t B, int T,
                                                 int Ta, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * Ta * n) return;
    if (Ta != 1) {
        da[e] = dP[e];
        return;
    }
    const int64_t b = e / n, k = e % n;
    const float* p = dP + b * T * n + k;
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += p[(int64_t)t * n];
    da[e] = acc;
}

// part[t][chunk] (J, J) = sum over the chunk's rows b of dQ[b, t] P[b, t]^T (contraction over the 4H
// columns, 32 at a time through LDS).  Thread (ty, tx) owns the outputs (ty + 16 p, tx + 16 q),
// p, q < TI (J <= 16 TI).
template <int TI>
__global__ __launch_bounds__(256) void k_lstm_dgx_part(const float* __restrict__ dQ, const float* __restrict__ P,
                                                       float* __restrict__ part, int64_t B, int T, int J, int H) {
    __shared__ float sd[16 * TI][33];
    __shared__ float sv[16 * TI][33];
    const int t = blockIdx.x, chunk = blockIdx.y, chunks = gridDim.y, H4 = 4 * H;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    float acc[TI][TI];
#pragma unroll
    for (int p = 0; p < TI; ++p)
#pragma unroll
        for (int q = 0; q < TI; ++q) acc[p][q] = 0.f;
    const int64_t b0 = (int64_t)chunk * kLstmDgxRows, b1 = min(B, b0 + kLstmDgxRows);
    for (int64_t b = b0; b < b1; ++b) {
        const float* V = P + lstm::at4(b, t, 0, T, J, H4);
        const float* D = dQ + lstm::at4(b, t, 0, T, J, H4);
        for (int n0 = 0; n0 < H4; n0 += 32) {  // H4 % 32 == 0 (H % 16 == 0)
            __syncthreads();
            for (int e = threadIdx.x; e < 16 * TI * 32; e += 256) {
                const int i = e >> 5, q = e & 31, n = n0 + q;
                const bool ok = i < J && n < H4;
                sd[i][q] = ok ? D[(int64_t)i * H4 + n] : 0.f;
                sv[i][q] = ok ? V[(int64_t)i * H4 + n] : 0.f;
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
    float* out = part + ((int64_t)t * chunks + chunk) * J * J;
#pragma unroll
    for (int p = 0; p < TI; ++p)
#pragma unroll
        for (int q = 0; q < TI; ++q) {
            const int i = ty + 16 * p, j = tx + 16 * q;
            if (i < J && j < J) out[i * J + j] = acc[p][q];
        }
}

// workspace layout: the backward's carve lies over the forward's bytes; a forward alone needs
// only its own (lstm_forward_bytes)
struct LstmWS {
    float *wt, *ptmp, *sbuf[2];                          // forward
    float *dQ, *dP, *cs, *dhc, *hp, *ident, *part, *gl;  // backward
    int64_t* types;
    size_t gl_bytes;
};

size_t lstm_carve(int64_t B, int T, int J, int H, int n_types, char* base, LstmWS* w, size_t* fwd_bytes = nullptr) {
    const int types = n_types > 0 ? n_types : 1;
    const size_t BJ = (size_t)B * J;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    LstmWS t{};
    LstmWS& o = w ? *w : t;
    // forward
    o.wt = (float*)take((size_t)types * 4 * H * H * sizeof(float));
    o.ptmp = (float*)take(BJ * 4 * H * sizeof(float));
    o.sbuf[0] = (float*)take(BJ * H * sizeof(float));
    o.sbuf[1] = (float*)take(BJ * H * sizeof(float));
    const size_t fwd = off;
    if (fwd_bytes) *fwd_bytes = fwd;
    // backward (over the same bytes)
    off = 0;
    o.dQ = (float*)take(BJ * T * 4 * H * sizeof(float));
    o.dP = (float*)take(BJ * T * 4 * H * sizeof(float));
    o.cs = (float*)take(BJ * H * sizeof(float));
    o.dhc = (float*)take(BJ * H * sizeof(float));
    o.hp = (float*)take(BJ * T * H * sizeof(float));
    o.ident = (float*)take((size_t)J * J * sizeof(float));
    o.types = (int64_t*)take((size_t)kMaxNodes * sizeof(int64_t));
    const size_t chunks = (size_t)((B + kLstmDgxRows - 1) / kLstmDgxRows);
    o.part = (float*)take((size_t)T * chunks * J * J * sizeof(float));
    o.gl_bytes = sd_gl_train_workspace_bytes(B * T, J, H, 4 * H, n_types);
    o.gl = (float*)take(o.gl_bytes);
    return off > fwd ? off : fwd;
}

}  // namespace
}  // namespace sd

extern "C" {

size_t sd_lstm_train_forward_workspace_bytes(int64_t rows, int32_t J, int32_t H, int32_t n_types) {
    if (rows < 0 || J < 1 || J > sd::kMaxNodes || H < 1 || n_types < 0) return 0;
    size_t fwd = 0;
    sd::lstm_carve(rows, 1, J, H, n_types, nullptr, nullptr, &fwd);
    return fwd;
}

size_t sd_lstm_train_workspace_bytes(int64_t rows, int32_t T, int32_t J, int32_t H, int32_t n_types) {
    if (rows < 0 || T < 1 || J < 1 || J > sd::kMaxNodes || H < 1 || n_types < 0) return 0;
    return sd::lstm_carve(rows, T, J, H, n_types, nullptr, nullptr);
}

int sd_lstm_train_forward(const float* a, int32_t Ta, const float* h0, const float* s0, const float* gx, int32_t Tg,
                          const float* W_hh, const float* b_hh, const int64_t* node_types, int32_t n_types, int64_t rows,
                          int32_t T, int32_t J, int32_t H, float* hs, float* s_last, float* P, float* gates, float* sseq,
                          void* workspace, size_t workspace_bytes, void* stream) {
    sd::NodeTypes nt;
    if (int rc = sd::seq_check("sd_lstm_train_forward", rows, T, Ta, Tg, J, H, node_types, n_types, false, &nt)) return rc;
    const bool keep = P || gates || sseq;
    if (keep && !(P && gates && sseq))
        return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: P, gates and sseq are kept together (all or none)");
    if (rows == 0) return SD_OK;
    if (!a) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: a is null");
    if (!h0) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: h0 is null");
    if (!s0) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: s0 is null");
    if (!gx) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: gx is null");
    if (!W_hh) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: W_hh is null");
    if (!hs) return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: hs is null");
    if (!workspace || workspace_bytes < sd_lstm_train_forward_workspace_bytes(rows, J, H, n_types))
        return sd::set_error(SD_E_INVALID, "sd_lstm_train_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    sd::LstmWS w;
    sd::lstm_carve(rows, T, J, H, n_types, (char*)workspace, &w);
    const int types = n_types > 0 ? n_types : 1;
    const int H4 = 4 * H;
    const int64_t JH = (int64_t)J * H, JH4 = (int64_t)J * H4;
    const int64_t nw = (int64_t)types * H4 * H;
    hipLaunchKernelGGL(sd::k_lstm_transpose_w, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, W_hh, (int64_t)types,
                       H, w.wt);
    SD_HIP(hipGetLastError());
    const int hh_threads = ((H4 < 1024 ? H4 : 1024) + 63) & ~63;
    const dim3 hh_grid((unsigned)J, (unsigned)((rows + sd::kLstmRT - 1) / sd::kLstmRT));
    const dim3 gate_grid((unsigned)rows, (unsigned)(H / sd::kLstmCH));
    for (int t = 0; t < T; ++t) {
        const float* hp = t == 0 ? h0 : hs + (int64_t)(t - 1) * JH;
        const int64_t hp_rs = t == 0 ? JH : (int64_t)T * JH;
        float* pt = keep ? P + (int64_t)t * JH4 : w.ptmp;
        const int64_t p_rs = keep ? (int64_t)T * JH4 : JH4;
        const float* at = a + (int64_t)sd::lstm::step_of(t, Ta) * JH4;
        hipLaunchKernelGGL(sd::k_lstm_hh, hh_grid, dim3(hh_threads), 0, s, at, (int64_t)Ta * JH4, hp, hp_rs, w.wt, b_hh, nt,
                           pt, p_rs, rows, J, H);
        SD_HIP(hipGetLastError());
        // s_{t-1}: s0, then the kept sequence or the workspace's two slabs in turn
        const float* sp = t == 0 ? s0 : (keep ? sseq + (int64_t)(t - 1) * JH : w.sbuf[(t - 1) & 1]);
        const int64_t sp_rs = (t > 0 && keep) ? (int64_t)T * JH : JH;
        const bool last = t == T - 1;
        float* so = keep ? sseq + (int64_t)t * JH : ((last && s_last) ? s_last : w.sbuf[t & 1]);
        const int64_t so_rs = keep ? (int64_t)T * JH : JH;
        float* so2 = (keep && last) ? s_last : nullptr;
        hipLaunchKernelGGL(sd::k_lstm_gate, gate_grid, dim3(256), 0, s, pt, p_rs, gx + sd::lstm::step_of(t, Tg) * J * J, sp,
                           sp_rs, hs + (int64_t)t * JH, (int64_t)T * JH, so, so_rs, so2, JH,
                           keep ? gates + (int64_t)t * JH4 : nullptr, (int64_t)T * JH4, J, H);
        SD_HIP(hipGetLastError());
    }
    return SD_OK;
}

int sd_lstm_train_backward(const float* dhs, int32_t Ta, const float* gx, int32_t Tg, const float* W_hh,
                           const int64_t* node_types, int32_t n_types, const float* h0, const float* s0, const float* hs,
                           const float* P, const float* gates, const float* sseq, int64_t rows, int32_t T, int32_t J,
                           int32_t H, float* da, float* dh0, float* ds0, float* dgx, float* dW_hh, float* db_hh,
                           void* workspace, size_t workspace_bytes, void* stream) {
    sd::NodeTypes nt;
    if (int rc = sd::seq_check("sd_lstm_train_backward", rows, T, Ta, Tg, J, H, node_types, n_types, dgx != nullptr, &nt)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int types = n_types > 0 ? n_types : 1;
    const int H4 = 4 * H;
    if (rows == 0) {  // empty batch: zero parameter gradients
        if (dgx) SD_HIP(hipMemsetAsync(dgx, 0, (size_t)Tg * J * J * sizeof(float), s));
        if (dW_hh) SD_HIP(hipMemsetAsync(dW_hh, 0, (size_t)types * H4 * H * sizeof(float), s));
        if (db_hh) SD_HIP(hipMemsetAsync(db_hh, 0, (size_t)types * H4 * sizeof(float), s));
        return SD_OK;
    }
    if (!dhs) return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: dhs is null");
    if (!gx) return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: gx is null");
    if (!W_hh) return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: W_hh is null");
    if (!h0 || !s0 || !hs) return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: h0, s0 or hs is null");
    if (!P || !gates || !sseq)
        return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: the forward's state (P, gates, sseq) is null");
    if (!workspace || workspace_bytes < sd_lstm_train_workspace_bytes(rows, T, J, H, n_types))
        return sd::set_error(SD_E_INVALID, "sd_lstm_train_backward: workspace too small");
    sd::LstmWS w;
    sd::lstm_carve(rows, T, J, H, n_types, (char*)workspace, &w);
    const int64_t JH = (int64_t)J * H, JH4 = (int64_t)J * H4;
    const dim3 hh_grid((unsigned)J, (unsigned)((rows + sd::kLstmRT - 1) / sd::kLstmRT));
    const unsigned ew_blocks = (unsigned)((rows * JH + 255) / 256);
    // reverse sweep
    for (int t = T - 1; t >= 0; --t) {
        hipLaunchKernelGGL(sd::k_lstm_gate_bwd, dim3(ew_blocks), dim3(256), 0, s, dhs, w.dhc, gates, sseq, s0, w.dQ, w.cs,
                           t == T - 1 ? 1 : 0, rows, T, t, J, H);
        SD_HIP(hipGetLastError());
        hipLaunchKernelGGL(sd::k_lstm_bwd_hh, hh_grid, dim3(256), 0, s, w.dQ, gx + sd::lstm::step_of(t, Tg) * J * J, W_hh,
                           nt, w.dP, w.dhc, rows, T, t, J, H);
        SD_HIP(hipGetLastError());
    }
    if (dh0) SD_HIP(hipMemcpyAsync(dh0, w.dhc, (size_t)rows * JH * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (ds0) SD_HIP(hipMemcpyAsync(ds0, w.cs, (size_t)rows * JH * sizeof(float), hipMemcpyDeviceToDevice, s));
    // batched over all rows x steps
    if (da) {
        const int64_t n = rows * Ta * JH4;
        hipLaunchKernelGGL(sd::k_lstm_da, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.dP, da, rows, T, Ta, JH4);
        SD_HIP(hipGetLastError());
    }
    if (dgx) {
        const int chunks = (int)((rows + sd::kLstmDgxRows - 1) / sd::kLstmDgxRows);
        const dim3 grid((unsigned)T, (unsigned)chunks);
        if (J <= 16)
            hipLaunchKernelGGL(sd::k_lstm_dgx_part<1>, grid, dim3(256), 0, s, w.dQ, P, w.part, rows, T, J, H);
        else if (J <= 32)
            hipLaunchKernelGGL(sd::k_lstm_dgx_part<2>, grid, dim3(256), 0, s, w.dQ, P, w.part, rows, T, J, H);
        else
            hipLaunchKernelGGL(sd::k_lstm_dgx_part<4>, grid, dim3(256), 0, s, w.dQ, P, w.part, rows, T, J, H);
        SD_HIP(hipGetLastError());
        const int cnt = (Tg == 1 ? T : 1) * chunks;
        const int64_t total = (int64_t)Tg * J * J;
        hipLaunchKernelGGL(sd::k_seq_dgx_sum, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, w.part, cnt, J * J,
                           total, dgx);
        SD_HIP(hipGetLastError());
    }
    if (dW_hh || db_hh) {
        // dW_hh = sum_{b,t} dP (x) h_{t-1}, db_hh = sum_{b,t} dP: the graph-linear's weight / bias
        // gradient over B T rows with an identity mixing matrix (one pass, fixed order)
        const int64_t n = rows * T * JH;
        hipLaunchKernelGGL(sd::k_lstm_hprev, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h0, hs, w.hp, rows, T, JH);
        SD_HIP(hipGetLastError());
        hipLaunchKernelGGL(sd::k_seq_identity, dim3((unsigned)((J * J + 255) / 256)), dim3(256), 0, s, w.ident, J);
        SD_HIP(hipGetLastError());
        if (n_types > 0) {
            hipLaunchKernelGGL(sd::k_seq_write_types, dim3(1), dim3(64), 0, s, nt, J, w.types);
            SD_HIP(hipGetLastError());
        }
        // (z feeds only dghat, which is not asked for; the entry still wants a non-null pointer)
        const int rc = sd_gl_train_backward(w.hp, P, w.dP, W_hh, n_types > 0 ? w.types : nullptr, n_types, w.ident,
                                            rows * T, J, H, H4, nullptr, dW_hh, db_hh, nullptr, w.gl, w.gl_bytes, stream);
        if (rc != SD_OK) return rc;
    }
    return SD_OK;
}

}  // extern "C"
