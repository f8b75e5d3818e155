// Layout of the sampling workspace (sd_workspace_bytes) and of the row chains that share it.  Plain
// C++: sd_plan.hip carves, shifts and sizes every buffer through this header and nothing else, and
// tests/host/workspace_layout_check.cpp includes it and walks the layout on the host.
//
// A buffer is `width` floats per (row, node); a padded buffer holds its rows rounded up to the 32-row
// blocks of the v4 layout.  Row chains (sd_plan.hip, record_loop) run rows [r0, r0 + n) of one call
// concurrently on separate streams, each on its own view of the same carve: the view starts r0 rows
// into every buffer and may touch ws_cap floats of it.  Offset and capacity come from the same
// width, so the views of two chains never overlap.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace sd {

// the Denoiser sizes the layout depends on (H = latent + cond dim, O = out dim, hid = heads * dim_head)
struct WsDims {
    int64_t J, H, D, O, hid;
    bool attention;
};

enum WsBuf { kWsRng, kWsX, kWsR, kWsH, kWsQkv, kWsO, kWsRes, kWsX0, kWsImg0, kWsImg1, kWsBufs };

struct WsSpec {
    int64_t width;  // floats per (row, node)
    bool pad32;     // rows padded to 32
    size_t fixed;   // bytes that do not scale with the rows
};

constexpr size_t kWsStatusByte = 32;  // the status word (sd_workspace_status) inside the rng block

// The table.  rng: {seed, row0} of the device noise and the status word.  qkv: to_qkv's output, and
// the split route's pre-mix Y scratch of every graph-linear outside the attention block (the widest
// layer's N: at least H).  o: the attention output; without attention the GL output (sized like x).
inline WsSpec ws_spec(const WsDims& d, int b) {
    switch (b) {
        case kWsRng: return {0, false, 64};
        case kWsX:
        case kWsR:
        case kWsH:
        case kWsRes: return {d.H, true, 0};
        case kWsQkv: return {std::max({d.attention ? 3 * d.hid : (int64_t)0, d.H, d.O}), true, 0};
        case kWsO: return {d.attention ? d.hid : d.H, true, 0};
        default: return {d.D, false, 0};  // x0, img0, img1: the latents, row-major
    }
}

inline size_t ws_align(size_t v) { return (v + 255) & ~(size_t)255; }

// floats of buffer b a call (or a chain) of n rows may touch: its carved size, and the capacity
// handed to the kernels (GLArgs::zs_cap for qkv)
inline int64_t ws_cap(const WsDims& d, int b, int64_t n) {
    const WsSpec s = ws_spec(d, b);
    return (s.pad32 ? (n + 31) / 32 * 32 : n) * d.J * s.width;
}
// float offset of row r0 of buffer b: where the view of a chain starting at r0 begins
inline int64_t ws_shift(const WsDims& d, int b, int64_t r0) { return r0 * d.J * ws_spec(d, b).width; }

struct WsCarve {
    size_t off[kWsBufs];  // byte offsets from the 256-B aligned base
    size_t bytes;
};
inline WsCarve ws_carve(const WsDims& d, int64_t rows) {
    WsCarve c{};
    for (int b = 0; b < kWsBufs; ++b) {
        c.off[b] = c.bytes;
        c.bytes += ws_align(ws_spec(d, b).fixed + (size_t)ws_cap(d, b, rows) * sizeof(float));
    }
    return c;
}

// Row chains.  Number of chains for `rows` rows (multiples of 32 rows each); opt: the plan's
// row_chains option, 0 = auto.  Every route runs with any chain count and the results are bitwise
// independent of it.
constexpr int kMaxChains = 8;
inline int chain_count(int opt, int64_t rows, int64_t split_rows) {
    // a partial last unit counts: 50 rows (config 4, one sequence) run as chains of 32 + 18 rows
    const int64_t units = (rows + 31) / 32;
    // auto (0): 3 chains (+ the caller's stream = HIP's default 4 hardware queues; a 4th chain
    // shares a queue: config 2 11.9k vs 15.9k futures/s), 2 on the small-batch split route
    // (400 rows: 5,920 vs 5,398 on one, 3,279 on three), one at 128 rows and below, where every
    // kernel is a few microseconds long and a second chain slows both (config 4, 50 rows: 61 vs
    // 106 futures/s; tools/sweep_routes.py, profiles/r03/ab)
    int n = opt > 0 ? std::min(opt, kMaxChains) : rows <= 128 ? 1 : rows <= split_rows ? 2 : 3;
    if (units < n) n = (int)std::max<int64_t>(1, units);
    return n;
}
inline int64_t chain_row(int i, int n, int64_t rows, int64_t unit) {
    return i >= n ? rows : std::min(rows, (rows + unit - 1) / unit * i / n * unit);
}

// Chain boundaries on the tiled route's GEMM tile.  k_gl4t's workgroup covers 256
// rows at RT = 2 (N <= 192) and 128 at RT = 1 (to_qkv), and a tile past the chain's rows still
// loads and multiplies (gl4t_body skips its stores only): cut on 32-row units, 3,200 rows on three
// chains are 33 / 33 / 34 tiles, 15 row groups of 256 where 12.5 hold data.  On kChainTileUnit
// rows the cuts leave whole waves / workgroups to all chains but the last.  Only where every chain
// keeps two full 256-row workgroups; below that the 32-row cuts stay (so do the small batches'
// chain shapes).  Rows are independent and the Philox rows / x_cond phase follow r0, so the
// results do not depend on where the cuts fall.
constexpr int64_t kChainTileUnit = 128;
static_assert(kChainTileUnit >= 32 && kChainTileUnit % 32 == 0, "chains start on 32-row blocks");
inline int64_t chain_start(int64_t rows, int n, int64_t unit, int i) {
    if (n < 1) n = 1;
    if (unit > 32) {
        if (unit % 32) unit = 32;
        for (int k = 0; k < n && unit > 32; ++k)
            if (chain_row(k + 1, n, rows, unit) - chain_row(k, n, rows, unit) < 512) unit = 32;
    } else {
        unit = 32;
    }
    return chain_row(i, n, rows, unit);
}

}  // namespace sd
