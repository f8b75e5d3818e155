// What the two recurrent training cores (sd_gru_train.hip, sd_lstm_train.hip) share: the node-type
// argument block, the small helper kernels of the batched gradients and the host-side argument
// checks.  Included inside each file's anonymous namespace in sd::, so every translation unit has
// its own copies.
#pragma once

constexpr int kSeqMaxH = 256;   // hidden width the per-step kernels' LDS tiles are sized for
constexpr int kSeqRT = 8;       // rows per workgroup of the per-node W_hh kernels
constexpr int kSeqDgxRows = 4;  // rows per partial of the dgx reduction

struct NodeTypes {
    int t[kMaxNodes];
};

__global__ void k_seq_write_types(NodeTypes nt, int J, int64_t* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < J) out[j] = nt.t[j];
}

__global__ void k_seq_identity(float* __restrict__ I, int J) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < J * J) I[k] = (k / J == k % J) ? 1.f : 0.f;
}

// dgx[g][e] = sum of `cnt` partials from part[g * cnt]: one wave per element, lane l takes the
// partials l, l + 64, ... in order, then a fixed xor-shuffle tree
__global__ __launch_bounds__(256) void k_seq_dgx_sum(const float* __restrict__ part, int cnt, int JJ, int64_t total,
                                                     float* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total) return;  // wave-uniform
    const int l = threadIdx.x & 63;
    const int64_t g = w / JJ;
    const int e = (int)(w % JJ);
    const float* p = part + g * cnt * JJ + e;
    float acc = 0.f;
    for (int s = l; s < cnt; s += 64) acc += p[(int64_t)s * JJ];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (l == 0) out[w] = acc;
}

// shared argument checks of the core entries; returns SD_OK or sets the error.  dgx_asked: the
// call launches the dgx partials, one grid row per kSeqDgxRows rows.
int seq_check(const char* fn, int64_t rows, int T, int Ta, int Tg, int J, int H, const int64_t* node_types, int n_types,
              bool dgx_asked, NodeTypes* nt) {
    const std::string f(fn);
    if (rows < 0) return set_error(SD_E_INVALID, f + ": rows < 0");
    if (T < 1) return set_error(SD_E_INVALID, f + ": T must be >= 1");
    if (J < 1 || J > kMaxNodes) return set_error(SD_E_INVALID, f + ": J outside 1..64");
    if (H < 16 || H % 16 != 0 || H > kSeqMaxH)
        return set_error(SD_E_INVALID, f + ": H must be a positive multiple of 16, at most 256");
    if (Ta != 1 && Ta != T) return set_error(SD_E_INVALID, f + ": Ta must be 1 or T");
    if (Tg != 1 && Tg != T) return set_error(SD_E_INVALID, f + ": Tg must be 1 or T");
    if (n_types < 0) return set_error(SD_E_INVALID, f + ": n_types < 0");
    if (n_types > 0 && !node_types) return set_error(SD_E_INVALID, f + ": node_types is null with n_types > 0");
    for (int j = 0; j < kMaxNodes; ++j) nt->t[j] = 0;
    if (n_types > 0)
        for (int j = 0; j < J; ++j) {
            if (node_types[j] < 0 || node_types[j] >= n_types)
                return set_error(SD_E_INVALID, f + ": node_types[" + std::to_string(j) + "] out of range");
            nt->t[j] = (int)node_types[j];
        }
    if (rows * (int64_t)T > INT32_MAX / 2 || (rows + kSeqRT - 1) / kSeqRT > 65535)
        return set_error(SD_E_INVALID, f + ": too many rows");
    if (dgx_asked && (rows + kSeqDgxRows - 1) / kSeqDgxRows > 65535)
        return set_error(SD_E_INVALID, f + ": too many rows for dgx (at most 262140)");
    return SD_OK;
}
