// FID on the device: the reference's MetricStorerFID (src/metrics/fid.py:91-129) runs every
// future through ClassifierForFID.get_fid_features (src/metrics/fid_classifier.py:38-53: nn.GRU(48, 128, 2)
// over the frames, then tanh(linear1(h_last))) and keeps the activations of the whole test set on the host.
// Here:
//   k_fid_pack      the classifier's weights into MFMA B-fragment order (once per call, 166 k floats);
//   k_fid_features  one persistent workgroup per tile of 32 futures: both GRU layers over all frames, then
//                   linear1 + tanh.  The hidden states live in LDS (as the next step's A operand) and in
//                   registers (for the z blend); the motion is read once, in the layout the pipeline holds
//                   it in; only the (rows, feat) features reach HBM;
//   k_fid_stats / k_fid_stats_reduce   (count, sum x, sum x x^T) of a batch of features in float64, added
//                   to a running state.
//
// Arithmetic.  All products run on the exact-f32 matrix instruction v_mfma_f32_32x32x2_f32: A[row][k] is
// the tile's x_t or h, B[k][col] a weight column; wave w owns hidden units 32 w .. 32 w + 31 of all three
// gates, so the gate math of an (row, unit) element never leaves its lane.  Sigmoid and tanh are the
// v_exp_f32 + v_rcp_f32 forms of the graph-linear kernels.
//
// Summation order.  An output element's k-sum is one accumulator chain in the order of the k groups below,
// input side first, then hidden side; a tile row is one row of the A operand and never meets another row.
// So a future's features do not depend on its position in the tile or on the batch it arrives in.  The
// statistics add rows in chunks of 256: a chunk's rows in row order (one thread per state entry), then the
// chunks in chunk order; no atomics.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skeldiff.h"
#include "sd_device.h"
#include "sd_internal.h"

namespace sd {

namespace {

constexpr int kH = 128;        // hidden size (the only one)
// 32-row MFMA tiles per workgroup.  The product is 1; -DSD_FID_ROW_TILES=2 builds the 64-row variant of the
// tile-height A/B (a diagnostic library, build_library(extra=...)): the same chains per row,
// each weight fragment used for two row tiles.
#ifndef SD_FID_ROW_TILES
#define SD_FID_ROW_TILES 1
#endif
constexpr int kRT = SD_FID_ROW_TILES;
static_assert(kRT == 1 || kRT == 2, "SD_FID_ROW_TILES");
constexpr int kTile = 32 * kRT;  // futures per workgroup
constexpr int kThreads = 256;  // 4 waves, wave w owns hidden units 32 w ..
constexpr int kMaxIn = 64, kMaxFeat = 32;
constexpr int kGH = kH / 8;    // k groups of 8 over the hidden size
constexpr int kFrag = 256;     // floats of one (k group, 32 columns) B fragment: 64 lanes x 4

// A-operand layout of a 32-row tile in LDS: element (row i, k) of a (32, 8 G) tile.  Lane (l32, h) of the
// MFMA reads the 16 bytes [k = 8 g + 4 h .. + 3] of row l32 for group g: one conflict-free ds_read_b128.
__device__ __forceinline__ int a_index(int i, int k) { return (((k >> 3) * 2 + ((k >> 2) & 1)) * 32 + i) * 4 + (k & 3); }

// packed weights (floats from the workspace base)
struct FidPack {
    int g0;  // k groups of the input side: ceil(input_size / 8)
    __host__ __device__ int wih0() const { return 0; }
    __host__ __device__ int whh0() const { return 12 * g0 * kFrag; }
    __host__ __device__ int wih1() const { return whh0() + 12 * kGH * kFrag; }
    __host__ __device__ int whh1() const { return wih1() + 12 * kGH * kFrag; }
    __host__ __device__ int lin() const { return whh1() + 12 * kGH * kFrag; }
    __host__ __device__ int bias() const { return lin() + kGH * kFrag; }  // [layer][r, z, in, hn][128], then linear1's [32]
    __host__ __device__ int total() const { return bias() + 2 * 4 * kH + kMaxFeat; }
};

struct FidWeights {
    const float *wih[2], *whh[2], *bih[2], *bhh[2], *lw, *lb;
    int K, feat;
};

// blockIdx.y: 0..3 the GRU matrices (ih0, hh0, ih1, hh1), 4 linear1, 5 the biases.
// Fragment (blk = wave * 3 + gate, g) holds, for lane (l32, h) and m = 0..3,
//   W[gate * 128 + wave * 32 + l32][8 g + 4 h + m]   (0 beyond the matrix: a padded K, a padded feat)
__global__ __launch_bounds__(kThreads) void k_fid_pack(FidWeights w, FidPack pk, float* __restrict__ out) {
    const int which = blockIdx.y;
    const int e0 = blockIdx.x * kThreads + threadIdx.x;
    if (which == 5) {
        if (e0 < 2 * 4 * kH) {
            const int layer = e0 / (4 * kH), q = (e0 / kH) & 3, j = e0 % kH;
            const float* bi = w.bih[layer];
            const float* bh = w.bhh[layer];
            float v;
            if (q == 0) v = bi[j] + bh[j];
            else if (q == 1) v = bi[kH + j] + bh[kH + j];
            else if (q == 2) v = bi[2 * kH + j];
            else v = bh[2 * kH + j];
            out[pk.bias() + e0] = v;
        } else if (e0 < 2 * 4 * kH + kMaxFeat) {
            const int j = e0 - 2 * 4 * kH;
            out[pk.bias() + e0] = j < w.feat ? w.lb[j] : 0.f;
        }
        return;
    }
    const bool gru = which < 4;
    const float* W = which == 0 ? w.wih[0] : which == 1 ? w.whh[0] : which == 2 ? w.wih[1] : which == 3 ? w.whh[1] : w.lw;
    const int K = which == 0 ? w.K : kH;
    const int G = which == 0 ? pk.g0 : kGH;
    const int nblk = gru ? 12 : 1;
    const int base = which == 0 ? pk.wih0() : which == 1 ? pk.whh0() : which == 2 ? pk.wih1() : which == 3 ? pk.whh1() : pk.lin();
    if (e0 >= nblk * G * kFrag) return;
    const int m = e0 & 3, lane = (e0 >> 2) & 63, bg = e0 >> 8;
    const int g = bg % G, blk = bg / G;
    const int l32 = lane & 31, h = lane >> 5;
    const int row = gru ? (blk % 3) * kH + (blk / 3) * 32 + l32 : l32;
    const int nrows = gru ? 3 * kH : w.feat;
    const int k = 8 * g + 4 * h + m;
    out[base + e0] = (row < nrows && k < K) ? W[(int64_t)row * K + k] : 0.f;
}

// sigmoid and tanh on v_exp_f32 + v_rcp_f32 (sd_graph_linear_v4.hip:tanh4); both saturate cleanly
__device__ __forceinline__ float sigmoid_rcp(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float tanh_rcp(float x) {
    const float e = __builtin_amdgcn_exp2f(2.0f * 1.44269504088896341f * x);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// acc_q += A (32 x 8 G, LDS) W_q^T for the wave's 32 units of the gates q = r, z, n: per k group one A
// fragment and three B fragments (coalesced 1 KiB loads of the packed weights), 12 MFMAs
// A: kRT row tiles, `astride` floats apart, that share the B fragments.
__device__ __forceinline__ void gemm3(const float* __restrict__ A, int astride, const float* __restrict__ Wp, int G,
                                      int lane, floatx16 (&ar)[kRT], floatx16 (&az)[kRT], floatx16 (&an)[kRT]) {
    const float* wr = Wp + lane * 4;
    const float* wz = wr + G * kFrag;
    const float* wn = wz + G * kFrag;
    const float* ap = A + lane * 4;
#pragma unroll 4
    for (int g = 0; g < G; ++g) {
        const floatx4 r = *reinterpret_cast<const floatx4*>(wr + g * kFrag);
        const floatx4 z = *reinterpret_cast<const floatx4*>(wz + g * kFrag);
        const floatx4 n = *reinterpret_cast<const floatx4*>(wn + g * kFrag);
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
            const floatx4 a = *reinterpret_cast<const floatx4*>(ap + rt * astride + g * kFrag);
            ar[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, r.x, ar[rt], 0, 0, 0);
            az[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, z.x, az[rt], 0, 0, 0);
            an[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, n.x, an[rt], 0, 0, 0);
            ar[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, r.y, ar[rt], 0, 0, 0);
            az[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, z.y, az[rt], 0, 0, 0);
            an[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, n.y, an[rt], 0, 0, 0);
            ar[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, r.z, ar[rt], 0, 0, 0);
            az[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, z.z, az[rt], 0, 0, 0);
            an[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, n.z, an[rt], 0, 0, 0);
            ar[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, r.w, ar[rt], 0, 0, 0);
            az[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, z.w, az[rt], 0, 0, 0);
            an[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, n.w, an[rt], 0, 0, 0);
        }
    }
}

// One GRU layer step of the tile for the wave's 32 units: torch.nn.GRU's cell,
//   r = s(W_ir x + W_hr h + (b_ir + b_hr)), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
//   h' = (1 - z) n + z h.
// xin / hin: the A tiles of the input and of h (LDS); hout: where h' goes as the next A tile (another
// buffer than hin: other waves still read hin); hreg: this lane's 16 elements of h, updated in place.
// The kRT row tiles of xin / hin / hout lie xstride / kGH * kFrag floats apart.
__device__ __forceinline__ void gru_layer(const float* __restrict__ xin, int xstride, int GX,
                                          const float* __restrict__ wih, const float* __restrict__ hin,
                                          const float* __restrict__ whh, float* __restrict__ hout,
                                          floatx16 (&hreg)[kRT], float br, float bz, float bin, float bhn, int lane,
                                          int col) {
    floatx16 ar[kRT] = {}, az[kRT] = {}, ain[kRT] = {}, ahn[kRT] = {};
    gemm3(xin, xstride, wih, GX, lane, ar, az, ain);
    gemm3(hin, kGH * kFrag, whh, kGH, lane, ar, az, ahn);
    const int hh = lane >> 5;
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float r = sigmoid_rcp(ar[rt][v] + br);
            const float z = sigmoid_rcp(az[rt][v] + bz);
            const float n = tanh_rcp((ain[rt][v] + bin) + r * (ahn[rt][v] + bhn));
            const float hn = (1.0f - z) * n + z * hreg[rt][v];
            hreg[rt][v] = hn;
            hout[rt * kGH * kFrag + a_index((v & 3) + 8 * (v >> 2) + 4 * hh, col)] = hn;  // accumulator row of register v
        }
}

// dynamic LDS: x tiles [2][kRT][g0 * 256], then h tiles [layer 2][buffer 2][kRT][kGH * 256]
__global__ __launch_bounds__(kThreads, kRT == 1 ? 2 : 1) void k_fid_features(const float* __restrict__ motion, int64_t rows, int frames,
                                                              int K, int feat, const float* __restrict__ h0,
                                                              const float* __restrict__ pack, FidPack pk,
                                                              float* __restrict__ feats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G0 = pk.g0;
    float* xs = lds;
    const int XT = kRT * G0 * kFrag;       // floats of one x buffer
    float* hs = lds + 2 * XT;
    constexpr int HT = kRT * kGH * kFrag;  // floats of one h buffer

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, hh = lane >> 5;
    const int col = wave * 32 + l32;  // this lane's hidden unit
    const int64_t row0 = (int64_t)blockIdx.x * kTile;

    // this lane's biases
    const float* bp = pack + pk.bias();
    const float b0r = bp[col], b0z = bp[kH + col], b0in = bp[2 * kH + col], b0hn = bp[3 * kH + col];
    const float b1r = bp[4 * kH + col], b1z = bp[5 * kH + col], b1in = bp[6 * kH + col], b1hn = bp[7 * kH + col];
    // the wave's packed weights: fragments (wave * 3 + gate, g)
    const float* wih0 = pack + pk.wih0() + wave * 3 * G0 * kFrag;
    const float* whh0 = pack + pk.whh0() + wave * 3 * kGH * kFrag;
    const float* wih1 = pack + pk.wih1() + wave * 3 * kGH * kFrag;
    const float* whh1 = pack + pk.whh1() + wave * 3 * kGH * kFrag;

    // initial hidden states: registers and buffer 0 of each layer
    floatx16 hr0[kRT], hr1[kRT];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int i = (v & 3) + 8 * (v >> 2) + 4 * hh;
            const int64_t row = row0 + 32 * rt + i;
            float a = 0.f, b = 0.f;
            if (h0 && row < rows) {
                a = h0[row * kH + col];
                b = h0[(rows + row) * kH + col];
            }
            hr0[rt][v] = a;
            hr1[rt][v] = b;
            hs[rt * kGH * kFrag + a_index(i, col)] = a;
            hs[2 * HT + rt * kGH * kFrag + a_index(i, col)] = b;
        }

    // x staging: thread (row xi = tid / 8, c = tid % 8) carries k = c + 8 q, q < G0, of its row of each row tile
    const int xi = tid >> 3, xc = tid & 7;
    bool xrow_ok[kRT];
    const float* xrow[kRT];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
        xrow_ok[rt] = row0 + 32 * rt + xi < rows;
        xrow[rt] = motion + (row0 + (xrow_ok[rt] ? 32 * rt + xi : 0)) * (int64_t)frames * K;
    }
    float xr[kRT][kMaxIn / 8];
    auto load_x = [&](int t) {
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
            for (int q = 0; q < kMaxIn / 8; ++q) {
                const int k = xc + 8 * q;
                xr[rt][q] = (q < G0 && xrow_ok[rt] && k < K) ? xrow[rt][(int64_t)t * K + k] : 0.f;
            }
    };
    auto store_x = [&](float* dst) {
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
            for (int q = 0; q < kMaxIn / 8; ++q)
                if (q < G0) dst[rt * G0 * kFrag + a_index(xi, xc + 8 * q)] = xr[rt][q];
    };
    load_x(0);
    store_x(xs);
    __syncthreads();

    for (int t = 0; t < frames; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        if (t + 1 < frames) load_x(t + 1);  // in flight under layer 0
        gru_layer(xs + cur * XT, G0 * kFrag, G0, wih0, hs + cur * HT, whh0, hs + nxt * HT, hr0, b0r, b0z, b0in, b0hn,
                  lane, col);
        if (t + 1 < frames) store_x(xs + nxt * XT);  // read next after the step's second barrier
        __syncthreads();
        gru_layer(hs + nxt * HT, kGH * kFrag, kGH, wih1, hs + 2 * HT + cur * HT, whh1, hs + 2 * HT + nxt * HT, hr1, b1r,
                  b1z, b1in, b1hn, lane, col);
        __syncthreads();
    }

    // features = tanh(linear1(h1)): one 32 x 32 tile per row tile, wave rt
    if (wave < kRT) {
        const float* A = hs + 2 * HT + (frames & 1) * HT + wave * kGH * kFrag + lane * 4;
        const float* W = pack + pk.lin() + lane * 4;
        floatx16 acc = {};
#pragma unroll 4
        for (int g = 0; g < kGH; ++g) {
            const floatx4 a = *reinterpret_cast<const floatx4*>(A + g * kFrag);
            const floatx4 w = *reinterpret_cast<const floatx4*>(W + g * kFrag);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
        }
        const float bl = bp[8 * kH + l32];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int64_t row = row0 + 32 * wave + (v & 3) + 8 * (v >> 2) + 4 * hh;
            if (row < rows && l32 < feat) feats[row * feat + l32] = tanh_rcp(acc[v] + bl);
        }
    }
}

// ---- statistics --------------------------------------------------------------------------------------
constexpr int kChunk = 256;  // rows per workgroup

// partial[chunk][e]: e < feat: sum_r x[r][e];  e = feat + a feat + b: sum_r x[r][a] x[r][b], rows in row order
__global__ __launch_bounds__(kThreads) void k_fid_stats(const float* __restrict__ feats, int64_t rows, int feat,
                                                        double* __restrict__ partial) {
    __shared__ float x[kChunk * kMaxFeat];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kChunk;
    const int n = (int)(rows - r0 < kChunk ? rows - r0 : kChunk);
    for (int i = tid; i < n * feat; i += kThreads) x[i] = feats[r0 * feat + i];
    __syncthreads();
    const int E = feat + feat * feat;
    for (int e = tid; e < E; e += kThreads) {
        double s = 0.0;
        if (e < feat) {
            for (int r = 0; r < n; ++r) s += (double)x[r * feat + e];
        } else {
            const int a = (e - feat) / feat, b = (e - feat) - a * feat;
            for (int r = 0; r < n; ++r) s += (double)x[r * feat + a] * (double)x[r * feat + b];
        }
        partial[(int64_t)blockIdx.x * E + e] = s;
    }
}

// state[1 + e] += the chunks' partials in chunk order; state[0] += rows
__global__ __launch_bounds__(kThreads) void k_fid_stats_reduce(const double* __restrict__ partial, int64_t nchunks,
                                                               int E, int64_t rows, double* __restrict__ state) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e == 0) state[0] += (double)rows;
    if (e >= E) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s += partial[c * E + e];
    state[1 + e] += s;
}

int hip_fail(const char* what, hipError_t e) { return set_error(SD_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

// the desc's shape, validated (0 on success, else the message is set)
int check_desc(const char* who, const sd_fid_classifier_desc* d) {
    const std::string w(who);
    if (!d) return set_error(SD_E_INVALID, w + ": desc is null");
    if (d->hidden_size != kH) return set_error(SD_E_INVALID, w + ": hidden_size must be 128");
    if (d->feat_size < 1 || d->feat_size > kMaxFeat) return set_error(SD_E_INVALID, w + ": feat_size must be in 1..32");
    if (d->input_size < 1 || d->input_size > kMaxIn) return set_error(SD_E_INVALID, w + ": input_size must be in 1..64");
    return SD_OK;
}

}  // namespace

}  // namespace sd

extern "C" {

size_t sd_fid_workspace_bytes(const sd_fid_classifier_desc* desc, int64_t rows) {
    using namespace sd;
    if (check_desc("fid_workspace_bytes", desc)) return 0;
    if (rows < 0) {
        set_error(SD_E_INVALID, "fid_workspace_bytes: rows must be >= 0");
        return 0;
    }
    const FidPack pk{(desc->input_size + 7) / 8};
    return (size_t)pk.total() * sizeof(float);
}

int sd_fid_features(const sd_fid_classifier_desc* desc, const float* motion, int64_t rows, int32_t frames,
                    const float* h0, float* feats, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace sd;
    if (int rc = check_desc("fid_features", desc)) return rc;
    if (frames < 1) return set_error(SD_E_INVALID, "fid_features: frames must be >= 1");
    if (rows < 0 || rows > (int64_t)INT32_MAX * kTile) return set_error(SD_E_INVALID, "fid_features: rows must be in 0..2^36");
    if (rows == 0) return SD_OK;
    const FidPack pk{(desc->input_size + 7) / 8};
    if (workspace_bytes < (size_t)pk.total() * sizeof(float))
        return set_error(SD_E_INVALID, "fid_features: workspace_bytes is below sd_fid_workspace_bytes");
    if (!workspace) return set_error(SD_E_INVALID, "fid_features: workspace is null");
    if (!motion) return set_error(SD_E_INVALID, "fid_features: motion is null");
    if (!feats) return set_error(SD_E_INVALID, "fid_features: feats is null");
    FidWeights w{{desc->weight_ih_l0, desc->weight_ih_l1}, {desc->weight_hh_l0, desc->weight_hh_l1},
                 {desc->bias_ih_l0, desc->bias_ih_l1},     {desc->bias_hh_l0, desc->bias_hh_l1},
                 desc->linear1_weight, desc->linear1_bias, desc->input_size, desc->feat_size};
    for (int l = 0; l < 2; ++l)
        if (!w.wih[l] || !w.whh[l] || !w.bih[l] || !w.bhh[l]) return set_error(SD_E_INVALID, "fid_features: a GRU weight is null");
    if (!w.lw || !w.lb) return set_error(SD_E_INVALID, "fid_features: linear1 is null");

    const hipStream_t s = (hipStream_t)stream;
    float* pack = static_cast<float*>(workspace);
    const int pack_blocks = (12 * kGH * kFrag + kThreads - 1) / kThreads;  // the largest of the six parts
    hipLaunchKernelGGL(k_fid_pack, dim3(pack_blocks, 6), dim3(kThreads), 0, s, w, pk, pack);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("k_fid_pack", e);
    const size_t lds = (size_t)kRT * (2 * pk.g0 * kFrag + 4 * kGH * kFrag) * sizeof(float);  // <= 80 KiB per row tile
    e = lds_opt_in(k_fid_features, lds);
    if (e != hipSuccess) return hip_fail("k_fid_features (LDS size)", e);
    const int64_t tiles = (rows + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_fid_features, dim3((unsigned)tiles), dim3(kThreads), lds, s, motion, rows, frames,
                       desc->input_size, desc->feat_size, h0, pack, pk, feats);
    e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_fid_features", e);
}

size_t sd_fid_stats_workspace_bytes(int64_t rows, int32_t feat) {
    using namespace sd;
    if (rows < 0 || feat < 1 || feat > kMaxFeat) {
        set_error(SD_E_INVALID, "fid_stats_workspace_bytes: rows must be >= 0 and feat in 1..32");
        return 0;
    }
    const int64_t nchunks = (rows + kChunk - 1) / kChunk;
    return (size_t)nchunks * (size_t)(feat + feat * feat) * sizeof(double);
}

int sd_fid_stats_update(const float* feats, int64_t rows, int32_t feat, double* state, void* workspace,
                        size_t workspace_bytes, void* stream) {
    using namespace sd;
    if (feat < 1 || feat > kMaxFeat) return set_error(SD_E_INVALID, "fid_stats_update: feat must be in 1..32");
    if (rows < 0 || rows > (int64_t)INT32_MAX * kChunk) return set_error(SD_E_INVALID, "fid_stats_update: rows must be in 0..2^39");
    if (rows == 0) return SD_OK;
    const int64_t nchunks = (rows + kChunk - 1) / kChunk;
    const int E = feat + feat * feat;
    if (workspace_bytes < (size_t)nchunks * E * sizeof(double))
        return set_error(SD_E_INVALID, "fid_stats_update: workspace_bytes is below sd_fid_stats_workspace_bytes");
    if (!workspace) return set_error(SD_E_INVALID, "fid_stats_update: workspace is null");
    if (!feats) return set_error(SD_E_INVALID, "fid_stats_update: feats is null");
    if (!state) return set_error(SD_E_INVALID, "fid_stats_update: state is null");
    const hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_fid_stats, dim3((unsigned)nchunks), dim3(kThreads), 0, s, feats, rows, feat, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("k_fid_stats", e);
    hipLaunchKernelGGL(k_fid_stats_reduce, dim3((E + kThreads - 1) / kThreads), dim3(kThreads), 0, s, partial, nchunks, E,
                       rows, state);
    e = hipGetLastError();
    return e == hipSuccess ? SD_OK : hip_fail("k_fid_stats_reduce", e);
}

}  // extern "C"
