// Internal interfaces between the host plan (sd_plan.hip) and the gfx950 kernels
// (sd_kernels.hip, sd_graph_linear*.hip).  Not part of the public ABI (see include/skeldiff.h).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <stdint.h>

namespace sd {

constexpr int kMaxNodes = 64;

// One StaticGraphLinear (graph_structural.py:30-43) with its fused epilogue:
//   y_j   = s_j * (W_type(j) [x1_j | x2_j]) + bias_type(j)        (s_j = 1/max(|x1_j|,1e-12) if RMS)
//   z_i   = sum_j Ghat[i][j] y_j
//   z     = z * (film[n] + 1) + film[H + n]      (ResnetBlock FiLM, attention.py:71-73)
//   z     = act(z)                               (tanh)
//   z    += res                                  (residual, attention.py:16 / :102)
struct GLArgs {
    const float* x1; int64_t x1_rs; int K1; int x1_div;   // row b reads x1 row (b + x1_row0) / x1_div
    int64_t x1_row0;                                      // 0 <= x1_row0 < x1_div (a row chunk's phase)
    int tile_hint;                                        // v4 tile <NW><RT><CT> when gl4_cfg is 0 (0: per shape)
    // per-launch kernel selection (the plan's options, sd_plan_set_option; the sd_test_set_* hooks
    // for the test entry points): generation 0 auto / 2..5 forced (1: an alias of 2), v4 tile
    // <NW><RT><CT> (0 auto), v4 weight staging 0 LDS-DMA (CU held exclusively) / 1 register-staged
    // (CU shareable)
    int variant, gl4_cfg, gl4_stage;
    // v4 split route (phase 1 GEMM per (tile, node) into the zs scratch, phase 2 mixing epilogue;
    // bitwise identical to the one-kernel route): 0 auto, 1 never, 2 k_gl4y, 3 k_gl4t, 4 k_gl4t
    // except for to_qkv + attention
    int split;
    // v5 (J > 21) mixing pass (SD_OPT_V5_MIX): 0 the matrix-core form k_gl5_mixm, 1 the VALU form
    // k_gl5_mix (the same j-ordered fmaf chains)
    int v5_valu;
    int64_t route_rows;  // rows of the whole sampling call on this device (row chains: all chains); 0 = B
    const float* x2; int64_t x2_rs; int K2;               // optional second input (cat along K)
    const float* W;                                       // (types, N, K1+K2), K contiguous
    const float* bias;                                    // (types, N) or null
    const float* G;                                       // (J, J) Ghat, row-major
    const float* film;                                    // (2N): [scale | shift] or null
    const float* ln_w; const float* ln_b;                 // (J) Block.norm LayerNorm over nodes (norm_type 'layer', v4 only) or null
    const float* res; int64_t res_rs;                     // (B, J, N) or null
    float* out; int64_t out_rs;                           // (B, J, N)
    int64_t B;
    int N;
    int J;
    int act;                                              // 0 none, 1 tanh
    int ntypes;                                           // number of node types (rows of W / N)
    int wrow[kMaxNodes];                                  // type(j) * N  (row offset into W)
    int ntype[kMaxNodes];                                 // type(j)
    // v4 only: W pre-split into f16 hi/lo B fragments (make_split_weights); null -> v4 unusable
    const _Float16* wsp; int wsp_nct; float wsp_unscale;
    int prec;  // v4 products: 0 f32-accurate (3 split f16 products), 1 half (x_hi W'_hi only)
    // fused to_qkv + Attention (launch_qkv_attention_v4): heads of 32 dims, q scale dh^-1/2
    int attn_heads; float attn_scale; int attn_order;
    // v4 only: operand / result layouts, 0 = row-major (B, J, F), 1 = row-blocked (blk_off in
    // sd_graph_linear_v4.hip; rows padded to 32)
    int x1_blk, x2_blk, res_blk, out_blk;
    // v5: scratch for the pre-mix activations when res aliases out (zs_cap floats), or null;
    // v4 split route: the pre-mix Y of phase 1
    float* zs; int64_t zs_cap;
    // v4: bit 0 set (atomicOr) when an activation is outside the f16 range of the split
    // (|x| >= 65504: x_hi would be inf); null = not checked
    unsigned* status;
    // bf16 storage of operands / result (precision mode 2): the tensor
    // holds bf16 elements at the same element offsets (row-major only)
    int x1_bf16, x2_bf16, res_bf16, out_bf16;
    // v5 only (J > 21): run the GEMM phase alone and leave the pre-mix Y in `out` (k_attention_mix
    // mixes the to_qkv layer); hipErrorNotSupported where the route cannot
    int skip_mix = 0;
    // v4 tiled split route, two sibling layers over one input in one launch per phase
    // (launch_graph_linear_pair_v4).  GEMM phase (the pair's args): N = 2 pair_n columns, the
    // weight fragments and biases of both layers side by side; the column groups of the second
    // half take its own scale wsp_unscale2 and, on the exact-f32 fallback, its weights W2.
    // Mixing phase (each layer's own args): its Y is columns zs_c0 .. zs_c0 + N - 1 of a scratch
    // zs_n columns wide (0: N).
    int pair_n = 0;
    const float* W2 = nullptr;
    float wsp_unscale2 = 1.f;
    int zs_n = 0, zs_c0 = 0;
    // The struct is a kernel argument, and its size stays a whole number of 64-B lines: at 8 bytes
    // less (a removed member) every launch of the small-batch routes measured about 0.3 us longer,
    // 1.2 - 1.8 % of a 400- or 50-row step
    int line_pad_[2] = {0, 0};
};
static_assert(sizeof(GLArgs) % 64 == 0, "GLArgs: a whole number of 64-B lines (see line_pad_)");

// Kernels a sampling call launched (SD_OPT_LAST_ROUTE): every graph-linear / attention launch site
// ORs its bit into this host thread's word while run_denoiser records (eager) or captures (graph).
enum RouteBits : unsigned {
    kRouteOneKernel = 1,   // k_gl4 MODE 0: one-kernel graph-linear tile
    kRouteFusedAttn = 2,   // k_gl4 MODE 1: one-kernel to_qkv + attention
    kRouteGemmWave = 4,    // k_gl4y: small-batch split route, GEMM phase
    kRouteGemmTiled = 8,   // k_gl4t: tiled split route (and v5) GEMM phase
    kRouteMixPhase = 16,   // k_gl4 MODE 2 / 3: split-route mixing / attention phase
    kRouteV5Mix = 32,      // k_gl5_gemm / k_gl5_mix (J > 21)
    kRouteExact = 64,      // exact-f32 generations v2 (also what variant 1 runs) and v3
    kRouteAttention = 128,  // k_attention: the separate attention kernel (J > 21, unfused routes)
    // 256 / 512: round 5's small-batch fused tile and fused layer kernel (removed in round 6)
    kRouteAttnMix = 1024     // k_attention_mix: the to_qkv layer's mixing inside the attention kernel
};
extern thread_local unsigned g_route_bits;

// f16 hi/lo split of a (types, N, K) f32 weight in MFMA B-fragment order (sd_graph_linear_v4.hip)
struct SplitW {
    _Float16* w = nullptr;  // device, owned by the caller (hipFree)
    int nct = 0;            // 32-column tiles in the layout (padded to a multiple of 6)
    float scale = 1.f;      // W' = W * scale (a power of two)
    float unscale = 1.f;    // 1 / scale
};
hipError_t make_split_weights(const float* W, int ntypes, int N, int K, SplitW* out, hipStream_t s);
// bf16 copy of W in the same B-fragment layout (the hi slots hold bf16(W), unscaled; precision 2)
hipError_t make_bf16_weights(const float* W, int ntypes, int N, int K, SplitW* out, hipStream_t s);

// Multi-head attention over joints (attention.py:122-136) from a (B, J, 3*heads*dh) qkv buffer.
struct AttnArgs {
    const float* qkv; float* out; int64_t B; int J; int heads; int dh; float scale;
    // SD_OPT_ATTENTION 2: qkv holds the to_qkv layer's PRE-mix Y and the kernel mixes it with this
    // (J, J) G-hat first (k_attention_mix, 49 <= J <= 52, dh 32); null: qkv is mixed
    const float* G = nullptr;
};

// Posterior mean + correlated noise step (nonisotropic.py:196-210 / isotropic.py:85-95).
struct UpdArgs {
    const float* x0; const float* xt;
    const float* eps; int64_t eps_rs;      // given noise rows (noise_mode 1)
    const float* C1; const float* C2; const float* U; const float* sig;   // step-t tables
    float c1s, c2s, sigs;                  // isotropic scalars
    int obj; float xa, xb;                 // isotropic pred_noise / pred_v (obj 1): x0 = xa x_t - xb act(out)
    int iso; int act; int noise_mode;      // noise_mode: 0 none (t == 0), 1 given, 2 Philox
    int clip;                              // 1: x0 clamped to [-1, 1] (clip_denoised, base.py:318-319)
    uint64_t seed; int64_t row0; int step; const uint64_t* rng_dev;  // rng_dev: {seed,row0} or null
    int64_t row_shift;                     // added to row0 (either source): a row chunk's first row
    float* out; float* out2; int64_t out2_rs;
    float* mean_out; int64_t mean_rs; float* noise_out; int64_t noise_rs;
    int64_t B; int J; int D;
    int x0_bf16, xt_bf16, out_bf16;  // bf16 latents (precision mode 2); out2 / records stay f32
    int elementwise;  // SD_OPT_UPDATE_KERNEL: 0 k_update_mfma where it applies, 1 the element-per-thread forms
};

hipError_t launch_graph_linear(const GLArgs& a, bool rms, hipStream_t s);     // dispatches v2..v5 (sd_graph_linear.hip)
hipError_t launch_graph_linear_v5(const GLArgs& a, bool rms, hipStream_t s);  // J > 21: GEMM + mixing pass
hipError_t launch_graph_linear_v2(const GLArgs& a, bool rms, hipStream_t s);
hipError_t launch_graph_linear_v3(const GLArgs& a, bool rms, hipStream_t s);  // J in {16,17,21}
hipError_t launch_graph_linear_v4(const GLArgs& a, bool rms, hipStream_t s);  // needs a.wsp
hipError_t launch_qkv_attention_v4(const GLArgs& a, bool rms, hipStream_t s);  // J <= 16, dh 32
// split-f16 GEMM phase (k_gl4y) into row-major z (B, J, N) with row stride z_rs (v5, J > 21)
hipError_t launch_gemm_split(const GLArgs& a, bool rms, float* z, int64_t z_rs, hipStream_t s);
// Rows (of the whole sampling call, all row chains) at or below which the v4 layers take the
// small-batch split route (k_gl4y) and an auto plan runs two row chains.  Measured (round 4, same
// box, T = 100, J = 16 f32, tools/sweep_routes.py, profiles/r04j/sweep.txt; k_gl4y with every
// chunk in flight): 800 rows 9,648 futures/s (k_gl4y, 2 chains) vs 7,737 (k_gl4t, 3); 1,600 rows
// 12,109 vs 12,172 (equal); 400 rows 6,165 vs 4,361.
constexpr int64_t kSplitRows = 1200;
int graph_linear_split_route(const GLArgs& a);  // v4 route of a layer: 0 one-kernel, 1 k_gl4y, 2 k_gl4t phases
// Layers a and b (same x1 | x2, K and N, no RMS) on the tiled split route as one k_gl4t launch
// over pr (N = 2 a.N: GLArgs::pair_n) and one mixing launch; bitwise equal to launching a and b
// one after the other.  graph_linear_pair_ok: whether the pair launches (else launch a and b).
bool graph_linear_pair_ok(const GLArgs& pr, const GLArgs& a, const GLArgs& b);
hipError_t launch_graph_linear_pair_v4(const GLArgs& pr, const GLArgs& a, const GLArgs& b, hipStream_t s);
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);
hipError_t launch_update(const UpdArgs& a, hipStream_t s);
hipError_t launch_mix_mfma(const float* z, const float* G, float* out, int64_t rows, int J, int N, bool transpose,
                           hipStream_t s);  // G-hat (or G-hat^T) mixing of (rows, J, N), v5's MFMA pass
hipError_t launch_noise_fill(float* out, int64_t rows, int64_t n_per_row, uint64_t seed,
                             int64_t row0, int step, const uint64_t* rng_dev, hipStream_t s,
                             int64_t row_shift = 0,   // row_shift: added to row0 (either source)
                             int out_bf16 = 0);       // out holds bf16 elements
// dst[r * dst_rs + i] = src[r * src_rs + i] (i < n; n % 4 == 0) with f32 <-> bf16 conversion
hipError_t launch_convert_rows(void* dst, int dst_bf16, int64_t dst_rs, const void* src, int src_bf16,
                               int64_t src_rs, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_philox_raw(uint32_t* out, int64_t rows, int64_t quads, uint64_t seed,
                             int64_t row0, int step, hipStream_t s);
hipError_t launch_set_rng(uint64_t* rng_dev, uint64_t seed, int64_t row0, hipStream_t s);
hipError_t launch_copy_rows(float* dst, int64_t dst_rs, const float* src, int64_t src_rs,
                            int64_t rows, int64_t n, hipStream_t s);
// row-blocked v4 activation layout -> row-major (rows, J, F)
hipError_t launch_unblock(float* out, const float* in, int64_t rows, int J, int F, hipStream_t s);

// plan-finalize helpers (one-time)
hipError_t launch_sinusoidal(float* emb, int T, int dim, float neg_scale, hipStream_t s);
hipError_t launch_linear(const float* x, int M, int K, const float* W, const float* b, int N,
                         float* y, int in_act, int out_act, hipStream_t s);
hipError_t launch_ghat(const float* G, float* Ghat, int J, int normalize, hipStream_t s);
// sets the thread-local message sd_last_error() returns; returns `code` (sd_plan.hip)
int set_error(int code, const std::string& msg);
// a HIP call in an entry point (a function returning an SD_E_* code): its failure is the function's
#define SD_HIP(x)                                                                                          \
    do {                                                                                                   \
        hipError_t e_ = (x);                                                                               \
        if (e_ != hipSuccess) return sd::set_error(SD_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)
hipError_t launch_fold_gain(const float* W, const float* g, float mult, float* out,
                            int64_t rows, int K, hipStream_t s);
hipError_t launch_sigma(const float* logvar, float* sig, int64_t n, hipStream_t s);

// The minimum over a sequence's samples in the metric kernels (sd_metrics.hip k_ade_fde, sd_realism.hip
// k_realism_reduce): the smallest of v[0..S) as torch.min, NaN if there is one
__device__ __forceinline__ float min_or_nan(const float* v, int S) {
    float m = v[0];
    for (int s = 1; s < S; ++s) {
        const float x = v[s];
        if (x != x || m != m) {
            m = __builtin_nanf("");
        } else if (x < m) {
            m = x;
        }
    }
    return m;
}

}  // namespace sd
