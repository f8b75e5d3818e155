// Stand-alone host check of the sampling workspace's layout (csrc/sd_workspace.h), built with
// -fsanitize=address,undefined by tests/test_workspace_layout_host.py.  For every shape of
//   J in {16, 17, 21, 51} x (D, C) in {(96, 96), (96, 0), (16, 0)} x attention in {off, heads x
//   dim_head (8, 32), (4, 64), (1, 32), (1, 16)} x rows in {1, 31, 32, 33, 50, 64, 129, 400, 1200,
//   1201, 3200} x row_chains 1..8 x cut unit in {32, kChainTileUnit}
// checked here:
//   (a) every buffer of the carve lies inside the carved size, behind the one before it, 256-B aligned;
//   (b) for every pair of row chains and every buffer, the extents the chains may touch -- the view's
//       start (ws_shift) plus the capacity the engine hands the kernels (ws_cap of the chain's rows) --
//       are disjoint;
//   (c) every chain's extent, the last one's included, ends inside the buffer;
//   (d) the status word is where sd_workspace_status reads it (a carve of 0 rows).
// The small shapes are also walked in memory: each chain fills its extents of a buffer of the carved
// size with its own mark, finds nobody else's there, and ASan sees every byte it touches.
//
// The rule the engine had before this header is restated below (parent_shift: the qkv view moved by
// to_qkv's 3 hid, or H without attention, while its capacity was max(3 hid, H, O)); under it (b) must
// fail exactly where attention is on, 3 hid < H and more than one chain runs -- heads (1, 32) and
// (1, 16) of the list -- so the check is known to see the defect it guards against.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_workspace.h"

using namespace sd;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            exit(1);                                      \
        }                                                 \
    } while (0)

constexpr int64_t kSplitRows = 1200;  // sd::kSplitRows (sd_internal.h), the auto chain count's threshold

struct Extent {
    int64_t lo, hi;  // floats of the buffer: [lo, hi)
};
static bool overlap(Extent a, Extent b) { return a.lo < b.hi && b.lo < a.hi; }

// where the parent commit's shift_ws put the view of a chain starting at r0
static int64_t parent_shift(const WsDims& d, int b, int64_t r0) {
    const int64_t width = b == kWsQkv ? (d.attention ? 3 * d.hid : d.H) : ws_spec(d, b).width;
    return r0 * d.J * width;
}

static long n_shapes = 0, n_walked = 0, n_parent_overlaps[5] = {0, 0, 0, 0, 0};

static void check_shape(const WsDims& d, int attn_case, int64_t rows, int opt_chains, int64_t unit) {
    const WsCarve c = ws_carve(d, rows);
    // (a)
    for (int b = 0; b < kWsBufs; ++b) {
        const size_t end = b + 1 < kWsBufs ? c.off[b + 1] : c.bytes;
        CHECK(c.off[b] % 256 == 0, "buffer %d not 256-B aligned", b);
        CHECK(c.off[b] + ws_spec(d, b).fixed + (size_t)ws_cap(d, b, rows) * sizeof(float) <= end, "buffer %d runs into the next", b);
    }
    CHECK(c.bytes % 256 == 0, "carved size");
    // (d)
    const WsCarve c0 = ws_carve(d, 0);
    CHECK(c.off[kWsRng] == c0.off[kWsRng] && kWsStatusByte + sizeof(unsigned) <= ws_spec(d, kWsRng).fixed &&
              c0.off[kWsRng] + kWsStatusByte + sizeof(unsigned) <= c0.bytes,
          "status word outside a 0-row carve");
    CHECK(ws_cap(d, kWsRng, rows) == 0 && ws_shift(d, kWsRng, 1024) == 0, "the rng block follows the rows");

    const int nch = chain_count(opt_chains, rows, kSplitRows);
    CHECK(nch >= 1 && nch <= kMaxChains && nch <= (rows + 31) / 32, "chain count %d", nch);
    int64_t r0[kMaxChains + 1];
    for (int i = 0; i <= nch; ++i) r0[i] = chain_start(rows, nch, unit, i);
    CHECK(r0[0] == 0 && r0[nch] == rows, "chains do not cover the rows");
    for (int i = 0; i < nch; ++i) CHECK(r0[i] % 32 == 0 && r0[i] < r0[i + 1], "chain %d: rows [%lld, %lld)", i, (long long)r0[i], (long long)r0[i + 1]);

    bool parent_overlaps = false;
    for (int b = kWsRng + 1; b < kWsBufs; ++b) {
        Extent e[kMaxChains], pe[kMaxChains];
        for (int i = 0; i < nch; ++i) {
            const int64_t cap = ws_cap(d, b, r0[i + 1] - r0[i]);
            e[i] = Extent{ws_shift(d, b, r0[i]), ws_shift(d, b, r0[i]) + cap};
            pe[i] = Extent{parent_shift(d, b, r0[i]), parent_shift(d, b, r0[i]) + cap};
            // (c)
            CHECK(e[i].lo >= 0 && e[i].hi <= ws_cap(d, b, rows), "buffer %d: chain %d of %d ends at float %lld of %lld", b, i, nch,
                  (long long)e[i].hi, (long long)ws_cap(d, b, rows));
        }
        // (b)
        for (int i = 0; i < nch; ++i)
            for (int k = i + 1; k < nch; ++k) {
                CHECK(!overlap(e[i], e[k]), "buffer %d: chains %d and %d of %d overlap (J %lld H %lld hid %lld rows %lld)", b, i, k, nch,
                      (long long)d.J, (long long)d.H, (long long)d.hid, (long long)rows);
                if (overlap(pe[i], pe[k])) {
                    CHECK(b == kWsQkv, "the parent's rule overlaps in buffer %d", b);
                    parent_overlaps = true;
                }
            }
    }
    const bool expect = d.attention && 3 * d.hid < d.H && nch > 1;
    CHECK(parent_overlaps == expect, "the parent's rule %s (J %lld H %lld hid %lld rows %lld chains %d)",
          expect ? "shows no overlap where one is known" : "overlaps where none is known", (long long)d.J, (long long)d.H,
          (long long)d.hid, (long long)rows, nch);
    n_parent_overlaps[attn_case] += parent_overlaps;
    ++n_shapes;

    // the small shapes in memory: every chain marks what it may touch
    if (rows > 64 || d.J > 17 || unit != 32 || opt_chains > 3) return;
    std::vector<unsigned char> mem(c.bytes, 0xff);
    for (int i = 0; i < nch; ++i)
        for (int b = kWsRng + 1; b < kWsBufs; ++b) {
            unsigned char* q = mem.data() + c.off[b] + ws_shift(d, b, r0[i]) * sizeof(float);
            const size_t n = (size_t)ws_cap(d, b, r0[i + 1] - r0[i]) * sizeof(float);
            for (size_t k = 0; k < n; k += 4093) CHECK(q[k] == 0xff, "buffer %d: chain %d finds a mark", b, i);
            CHECK(n == 0 || q[n - 1] == 0xff, "buffer %d: chain %d finds a mark at its end", b, i);
            memset(q, i, n);
        }
    ++n_walked;
}

int main() {
    const int Js[] = {16, 17, 21, 51};
    const int DC[][2] = {{96, 96}, {96, 0}, {16, 0}};
    const int attn[][2] = {{0, 0}, {8, 32}, {4, 64}, {1, 32}, {1, 16}};  // heads, dim_head; {0, 0}: off
    const int64_t rows[] = {1, 31, 32, 33, 50, 64, 129, 400, 1200, 1201, 3200};
    const int64_t units[] = {32, kChainTileUnit};
    for (int J : Js)
        for (auto& dc : DC)
            for (int a = 0; a < 5; ++a)
                for (int64_t r : rows)
                    for (int ch = 1; ch <= 8; ++ch)
                        for (int64_t u : units) {
                            const int64_t hid = (int64_t)attn[a][0] * attn[a][1];
                            check_shape(WsDims{J, dc[0] + dc[1], dc[0], dc[0], hid, a != 0}, a, r, ch, u);
                        }
    CHECK(n_parent_overlaps[0] == 0 && n_parent_overlaps[1] == 0 && n_parent_overlaps[2] == 0, "the parent's rule at wide heads");
    CHECK(n_parent_overlaps[3] > 0 && n_parent_overlaps[4] > 0, "the parent's rule passes at heads (1, 32) / (1, 16)");
    printf("workspace layout ok (%ld shapes, %ld walked in memory; parent rule: %ld overlapping at heads (1, 32), %ld at (1, 16))\n",
           n_shapes, n_walked, n_parent_overlaps[3], n_parent_overlaps[4]);
    return 0;
}
