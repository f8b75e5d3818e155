// Kernel-argument blocks of the v4 split route (sd_graph_linear_v4.hip) and the work-unit decode
// its kernels share with the host.
//
// GLArgs (sd_internal.h) stays the host-side description of a layer: 832 bytes, of which a GEMM-phase
// kernel reads about 200 and a mixing-phase kernel about 120.  The split route's kernels -- k_gl4t,
// k_gl4y, k_gl4 MODE 2 / 3 and k_gl4_pair, 213 launches per denoise step at config 2 -- take one of
// the compact blocks below instead, packed from GLArgs by the launchers (k_gl4t as its last parameter,
// YOut: sd_graph_linear_v4.hip).  Everything that is the same
// for every workgroup of a launch is worked out here, on the host: the grid factors as multiply-high
// reciprocals (no 64-bit division or modulo on the device before the first address), the XCD split
// of the grid, the resolved scratch width, the output strides.  A block's size is a whole number of
// 64-byte lines.
//
// Plain C++ apart from GLArgs itself: tests/host/launch_decode_check.cpp includes this header and
// checks the decode, the remap and the packers on the host.
#pragma once
#include <stdint.h>

#include "sd_internal.h"

#if defined(__HIPCC__)
#define SD_HD __host__ __device__ __forceinline__
#else
#define SD_HD inline
#endif

namespace sd {

// u / d and u % d for any 32-bit u and d >= 1 from one multiply-high and one correction:
// m = floor(2^32 / d) (d = 1: 2^32 - 1), q' = mulhi(u, m) is floor(u / d) or one less.
struct FastDiv {
    uint32_t d, m;
};
inline FastDiv make_fastdiv(uint32_t d) { return FastDiv{d, d <= 1 ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d)}; }
SD_HD void fast_divmod(uint32_t u, FastDiv f, uint32_t& q, uint32_t& r) {
    q = (uint32_t)(((uint64_t)u * f.m) >> 32);
    r = u - q * f.d;
    if (r >= f.d) {
        ++q;
        r -= f.d;
    }
}

// Work unit u of a grid ordered (lo fastest, then mid, then hi): lo = u % a, mid = (u / a) % b,
// hi = (u / a) / b.
//   k_gl4t: a = column groups, b = row groups       -> lo = column group, mid = row group, hi = node
//   k_gl4y: a = 32-column tiles, b = nodes (J)      -> lo = column tile, mid = node, hi = row tile
struct Unit3 {
    uint32_t lo, mid, hi;
};
SD_HD Unit3 decode_unit(uint32_t u, FastDiv a, FastDiv b) {
    Unit3 r;
    uint32_t t;
    fast_divmod(u, a, t, r.lo);
    fast_divmod(t, b, r.hi, r.mid);
    return r;
}

// XCD-aware order (cdna_hip_programming.md §5.5 T1) of k_gl4t, the one-kernel k_gl4, k_gl3 and k_gl2:
// workgroups b, b + 8, ... run on one XCD and take a contiguous share of the units, so the column groups
// of one (row group, node) -- which read the same x -- meet in one L2.  q8 = grid / 8, r8 = grid % 8: the
// first r8 XCDs take q8 + 1 units.  Bijective for any grid size.
SD_HD uint32_t xcd_remap(uint32_t block, uint32_t q8, uint32_t r8) {
    const uint32_t xcd = block & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (block >> 3);
}

// 64-byte lines of padding on every block: 0 and 1 measured the same at 50, 800 and 3,200 rows
// (DESIGN.md §4v), so the blocks keep their smallest whole-line size
constexpr int kGl4ArgsPadLines = 0;

// GEMM phase: k_gl4t and k_gl4y.  The Y tile (row tile tr, node j, column tile t) starts at
// y + tr y_ts + j y_js + t y_cs; inside it, the scratch's block layout or rows y_rs apart
// (sd_ystore_map.h).  The first three lines hold what a workgroup needs
// before its first operand load (gl4g_preload: one batch of scalar loads, one wait); the last line
// what only the stores and the exact-f32 fallback read.
struct GL4GArgs {
    FastDiv da, db;     // decode_unit's factors
    uint32_t q8, r8;    // xcd_remap's (k_gl4t)
    int J, N;
    const _Float16* wsp;
    const float* x1;
    const float* x2;
    const float* bias;
    int64_t B, ntile_r;
    int K1, K2, wsp_nct, pair_n;
    uint8_t x1_blk, x2_blk, x1_bf16, x2_bf16;
    int x1_div;
    int64_t x1_rs, x2_rs, x1_row0;
    uint32_t ntype4[kMaxNodes / 4];  // type(j), one byte per node
    float* y;
    int64_t y_ts;
    int y_rs, y_js, y_cs;
    float wsp_unscale, wsp_unscale2;
    int line_pad_[kGl4ArgsPadLines * 16 + 1];
    const float* W;   // exact-f32 fallback (f16 range left)
    const float* W2;  // ... of a paired launch's second layer
    unsigned* status;
};
// type(j) by selection over the whole table: every word arrives with the block's first loads, so no
// load depends on the decoded node
SD_HD int gl4_node_type(const GL4GArgs& p, int j) {
    uint32_t w = p.ntype4[0];
#pragma unroll
    for (int i = 1; i < kMaxNodes / 4; ++i) w = (j >> 2) == i ? p.ntype4[i] : w;
    return (int)((w >> ((j & 3) * 8)) & 0xFFu);
}

// Mixing phase: k_gl4 MODE 2 (mixing, FiLM / tanh / residual) and MODE 3 (attention epilogue).
struct GL4MArgs {
    const float* zs;  // the GEMM phase's Y (zs_off), zs_n columns wide; this layer's start at zs_c0
    const float* G;
    const float* film;
    const float* ln_w;
    const float* ln_b;
    const float* res;
    float* out;
    int64_t B, res_rs, out_rs;
    int N, zs_n, zs_c0, act, attn_heads;
    float attn_scale;
    FastDiv ntc;  // column tiles of a row tile (MODE 2: N / 32, MODE 3: heads)
    uint8_t res_blk, out_blk, res_bf16, out_bf16;
    int line_pad_[kGl4ArgsPadLines * 16 + 3];
};
// two layers behind one paired GEMM launch: nta column tiles of a, then ntb of b, per row tile
struct GL4PairArgs {
    GL4MArgs a, b;
    FastDiv nt;  // nta + ntb
    uint32_t nta;
    int line_pad_[13];
};
static_assert(sizeof(GL4GArgs) % 64 == 0 && sizeof(GL4GArgs) == 256 + 64 * kGl4ArgsPadLines, "GL4GArgs: whole 64-B lines");
static_assert(sizeof(GL4MArgs) % 64 == 0 && sizeof(GL4MArgs) == 128 + 64 * kGl4ArgsPadLines, "GL4MArgs: whole 64-B lines");
static_assert(sizeof(GL4PairArgs) % 64 == 0, "GL4PairArgs: whole 64-B lines");

// A grid of `units` 32-bit work units (the decode is 32-bit; gridDim.x is at most 2^31 - 1)
inline bool gl4_grid_ok(int64_t units) { return units > 0 && units < (int64_t)1 << 31; }

// The GEMM-phase block of layer a writing through (y, strides).  a_div / b_div: decode_unit's factors
// (k_gl4t: column groups, row groups; k_gl4y: column tiles, J); grid: workgroups of the launch.
// false: a value does not fit its field (the launcher refuses the launch).
inline bool pack_gl4g(const GLArgs& a, int64_t ntile_r, float* y, int64_t y_rs, int64_t y_js, int64_t y_ts, int64_t y_cs,
                      uint32_t a_div, uint32_t b_div, uint32_t grid, GL4GArgs* o) {
    *o = GL4GArgs{};
    if (a.J < 1 || a.J > kMaxNodes || a_div < 1 || b_div < 1) return false;
    if (y_rs < 0 || y_js < 0 || y_cs < 0 || y_rs > INT32_MAX || y_js > INT32_MAX || y_cs > INT32_MAX) return false;
    o->x1 = a.x1; o->x2 = a.x2; o->wsp = a.wsp; o->bias = a.bias; o->W = a.W; o->W2 = a.W2; o->status = a.status; o->y = y;
    o->x1_rs = a.x1_rs; o->x2_rs = a.x2_rs; o->x1_row0 = a.x1_row0; o->B = a.B; o->ntile_r = ntile_r; o->y_ts = y_ts;
    o->y_rs = (int)y_rs; o->y_js = (int)y_js; o->y_cs = (int)y_cs;
    o->K1 = a.K1; o->K2 = a.K2; o->x1_div = a.x1_div; o->N = a.N; o->J = a.J; o->pair_n = a.pair_n; o->wsp_nct = a.wsp_nct;
    o->wsp_unscale = a.wsp_unscale; o->wsp_unscale2 = a.wsp_unscale2;
    o->da = make_fastdiv(a_div); o->db = make_fastdiv(b_div);
    o->q8 = grid >> 3; o->r8 = grid & 7;
    o->x1_blk = a.x1_blk != 0; o->x2_blk = a.x2_blk != 0; o->x1_bf16 = a.x1_bf16 != 0; o->x2_bf16 = a.x2_bf16 != 0;
    for (int j = 0; j < a.J; ++j) {
        // wrow is type * N everywhere a GLArgs is filled; the kernels rebuild it from the type
        if (a.ntype[j] < 0 || a.ntype[j] > 255 || a.wrow[j] != a.ntype[j] * a.N) return false;
        o->ntype4[j >> 2] |= (uint32_t)a.ntype[j] << ((j & 3) * 8);
    }
    return true;
}

// The mixing-phase block of layer a; ntc: column tiles per row tile (MODE 2: N / 32, MODE 3: heads)
inline bool pack_gl4m(const GLArgs& a, uint32_t ntc, GL4MArgs* o) {
    *o = GL4MArgs{};
    if (ntc < 1) return false;
    o->zs = a.zs; o->G = a.G; o->film = a.film; o->ln_w = a.ln_w; o->ln_b = a.ln_b; o->res = a.res; o->out = a.out;
    o->B = a.B; o->res_rs = a.res_rs; o->out_rs = a.out_rs;
    o->N = a.N; o->zs_n = a.zs_n ? a.zs_n : a.N; o->zs_c0 = a.zs_c0; o->act = a.act; o->attn_heads = a.attn_heads;
    o->attn_scale = a.attn_scale;
    o->ntc = make_fastdiv(ntc);
    o->res_blk = a.res_blk != 0; o->out_blk = a.out_blk != 0; o->res_bf16 = a.res_bf16 != 0; o->out_bf16 = a.out_bf16 != 0;
    return true;
}

inline bool pack_gl4_pair(const GLArgs& a, const GLArgs& b, GL4PairArgs* o) {
    *o = GL4PairArgs{};
    if (a.N < 32 || b.N < 32 || (a.N & 31) || (b.N & 31)) return false;
    if (!pack_gl4m(a, (uint32_t)(a.N >> 5), &o->a) || !pack_gl4m(b, (uint32_t)(b.N >> 5), &o->b)) return false;
    o->nta = (uint32_t)(a.N >> 5);
    o->nt = make_fastdiv((uint32_t)((a.N + b.N) >> 5));
    return true;
}

}  // namespace sd
