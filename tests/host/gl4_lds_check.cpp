// Stand-alone host check of the v4 graph-linear tile's dynamic LDS layout (csrc/sd_gl4_lds.h), built
// with -fsanitize=address,undefined by tests/test_gl4_lds_host.py.  For every (J, CT, MODE, PREC) that
// sd_graph_linear_v4.hip can instantiate (tiles() below) and ntypes 1..J:
//   (a) the total bytes are what the launchers computed before the header (old_bytes: gl4_launch_t's
//       wfl / yfl / lds; old_pair_bytes: gl4_pair's literal), and two values are pinned;
//   (b) the regions a mode uses at the same time are disjoint and end inside the total: the two weight
//       stages, Y and Z (MODE 1: side by side; MODE 3, and only MODE 3: Z over Y), G-hat and FiLM
//       behind max(stages, Y + Z);
//   (c) the largest float offset a lane can form from the slab strides lies inside its region: the
//       mixing A position (a_off, every block b < COLS, lane lr, both output layouts), the
//       accumulator exchange, the slab pieces phase 2's slab load writes (MODE 2 and MODE 3's dst, every
//       q < YQ), the Z pieces of the attention epilogue.  The offsets are also written into a buffer
//       of exactly the region's size, so ASan sees each one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_device.h"
#include "../../skeletondiffusion_amd/csrc/sd_gl4_lds.h"
#include "../../skeletondiffusion_amd/csrc/sd_ystore_map.h"

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

// gl4_body's a_off (MODE 0 / 2), restated: offset in a node's slab (row YR + column) of the A position that lane lr (0..15) reads
// for mixing block b (0 <= b < COLS).  A block is 16 (row, column) positions: row-major output, 16
// consecutive columns of one row; row-blocked output (blk_out), 4 rows x 4 columns.
static int mix_a_off(int COLS, int YR, bool blk_out, int b, int lr) {
    return blk_out ? ((b / (COLS / 4)) * 4 + (lr >> 2)) * YR + (b % (COLS / 4)) * 4 + (lr & 3)
                   : (b / (COLS / 16)) * YR + (b % (COLS / 16)) * 16 + lr;
}

// the old rule: gl4_launch_t before sd_gl4_lds.h
static size_t old_bytes(int J, int CT, int MODE, int PREC, int ntypes) {
    const int COLS = 32 * CT;
    const bool ATT = MODE == 1 || MODE == 3;
    const size_t wfl = MODE >= 2 ? 0 : (size_t)ntypes * CT * (PREC ? 512 : 1024);
    const size_t y8 = (size_t)J * (8 * COLS + 16), z8 = (size_t)8 * J * 100;
    const size_t yfl = MODE == 3 ? (y8 > z8 ? y8 : z8) : ATT ? y8 + z8 : (size_t)J * (16 * (COLS + 4) + 16);
    return ((wfl > yfl ? wfl : yfl) + (size_t)J * J + 2 * COLS) * sizeof(float);
}
// ... and gl4_pair's literal
static size_t old_pair_bytes(int J) { return ((size_t)J * (16 * 36 + 16) + (size_t)J * J + 64) * sizeof(float); }

struct Tile {
    int J, CT, MODE, PREC;
};
// Every tile gl4_body's static_asserts admit at the J of with_J, whether or not a launcher picks it today:
// MODE 0 with 1..3 column tiles, MODE 1 / 3 a head's three, MODE 2 one; the three precisions.  (No table
// of the file's instantiations to keep in step; tests/test_gl4_lds_host.py checks that the file stays inside.)
static std::vector<Tile> tiles() {
    std::vector<Tile> t;
    for (int J : {16, 17, 21})
        for (int PREC : {0, 1, 2}) {
            for (int CT : {1, 2, 3}) t.push_back({J, CT, 0, PREC});
            t.push_back({J, 3, 1, PREC});
            t.push_back({J, 1, 2, PREC});
            t.push_back({J, 3, 3, PREC});
        }
    return t;
}

struct Region {
    const char* name;
    long lo, hi;  // floats: [lo, hi)
};
static bool overlap(const Region& a, const Region& b) { return a.lo < b.hi && b.lo < a.hi; }

static long n_layouts = 0, n_offsets = 0;

// offset `off` (a run of `n` floats) inside a region of `size` floats; `mem` has exactly that size
static void touch(std::vector<float>& mem, long off, int n, const char* what, const Tile& t) {
    CHECK(off >= 0 && off + n <= (long)mem.size(), "%s: offset %ld + %d outside %zu floats (J %d CT %d MODE %d)", what, off, n,
          mem.size(), t.J, t.CT, t.MODE);
    for (int i = 0; i < n; ++i) mem.data()[off + i] = 1.0f;
    ++n_offsets;
}

static void check_tile(const Tile& t, int ntypes) {
    const int J = t.J, MODE = t.MODE;
    const Gl4Lds L = gl4_lds(J, t.CT, MODE, t.PREC, ntypes);
    const bool att = MODE == 1 || MODE == 3;
    ++n_layouts;
    // (a)
    CHECK(L.bytes == old_bytes(J, t.CT, MODE, t.PREC, ntypes), "bytes %zu, old rule %zu (J %d CT %d MODE %d PREC %d ntypes %d)", L.bytes,
          old_bytes(J, t.CT, MODE, t.PREC, ntypes), J, t.CT, MODE, t.PREC, ntypes);
    if (MODE == 2) CHECK(L.bytes == old_pair_bytes(J), "MODE 2 bytes %zu, gl4_pair's literal %zu", L.bytes, old_pair_bytes(J));
    CHECK(L.COLS == 32 * t.CT, "COLS");
    // (b)
    const long total = (long)(L.bytes / sizeof(float));
    const long stage_fl = L.stage_h / 2;  // one stage, in floats
    CHECK((MODE < 2) == (L.stage_h > 0) && L.stage_h % 8 == 0, "weight stages: the K loop's modes only, whole 16-B pieces");
    std::vector<Region> live_k = {{"stage 0", 0, stage_fl}, {"stage 1", stage_fl, 2 * stage_fl}};  // during the K loop
    std::vector<Region> live_e = {{"Y", L.sY, L.sY + L.y_floats}};                                  // during the epilogue
    CHECK(att == (L.sZ >= 0) && att == (L.z_floats > 0), "Z: the attention modes only");
    if (att) {
        const Region z{"Z", L.sZ, L.sZ + L.z_floats};
        if (MODE == 3) CHECK(L.sZ == L.sY, "MODE 3: Z over Y");
        else CHECK(!overlap(live_e[0], z), "MODE 1: Y and Z overlap");  // aliasing in MODE 3 only
        if (MODE != 3) live_e.push_back(z);
        else live_e[0].hi = live_e[0].hi > z.hi ? live_e[0].hi : z.hi;
        CHECK(L.sZ % 4 == 0 && L.ZN % 4 == 0 && L.ZR % 4 == 0, "Z: 16-B pieces");
    }
    const Region g{"G-hat", L.sG, L.sG + J * J}, f{"FiLM", L.sF, L.sF + 2 * L.COLS};
    for (auto* live : {&live_k, &live_e}) {  // G-hat and FiLM are written before the K loop and read after it
        live->push_back(g);
        live->push_back(f);
        for (size_t i = 0; i < live->size(); ++i) {
            CHECK((*live)[i].lo >= 0 && (*live)[i].hi <= total, "%s ends outside the total", (*live)[i].name);
            for (size_t k = i + 1; k < live->size(); ++k)
                CHECK(!overlap((*live)[i], (*live)[k]), "%s and %s overlap (J %d CT %d MODE %d ntypes %d)", (*live)[i].name,
                      (*live)[k].name, J, t.CT, MODE, ntypes);
        }
    }
    CHECK(f.hi == total, "FiLM: last");
    if (ntypes > 1) return;  // (c) does not depend on ntypes
    // (c)
    std::vector<float> y((size_t)L.y_floats, 0.f);
    if (!att) {
        CHECK(L.YR % 4 == 0 && L.YS % 4 == 0, "slab: 16-B pieces");
        for (int blk = 0; blk < 2; ++blk)
            for (int b = 0; b < L.COLS; ++b)
                for (int lr = 0; lr < 16; ++lr)
                    for (int jj = 0; jj < J; ++jj) touch(y, (long)jj * L.YS + mix_a_off(L.COLS, L.YR, blk != 0, b, lr), 1, "a_off", t);
        if (MODE == 0)  // the accumulator exchange: node j, row r, column 32 ct + l32
            for (int j = 0; j < J; ++j)
                for (int r = 0; r < 16; ++r)
                    for (int c = 0; c < L.COLS; ++c) touch(y, (long)j * L.YS + r * L.YR + c, 1, "exchange", t);
        if (MODE == 2) {  // phase 2's slab load: piece q of the slab
            const int C4 = L.COLS / 4, YQ = J * 16 * C4;
            for (int q = 0; q < YQ; ++q) {
                int r, cc;
                zs_slab_piece(q % (16 * C4), 16, &r, &cc);
                touch(y, (long)(q / (16 * C4)) * L.YS + r * L.YR + cc, 4, "MODE 2 dst", t);
            }
        }
    } else {
        CHECK(L.YS8 % 4 == 0 && L.COLS == 96, "8-row slab: 16-B pieces, q | k | v");
        if (MODE == 1)  // attention_epilogue's exchange: node j, row e + 4 h, column 32 ct + l32
            for (int j = 0; j < J; ++j)
                for (int r = 0; r < 8; ++r)
                    for (int c = 0; c < L.COLS; ++c) touch(y, (long)j * L.YS8 + r * L.COLS + c, 1, "exchange 8", t);
        if (MODE == 3) {  // phase 2's slab load, dst
            const int YQ = J * 8 * 24;
            for (int q = 0; q < YQ; ++q) {
                const int j = (q >> 6) % J, ct = (q >> 6) / J;
                int rr, cc;
                zs_slab_piece(q & 63, 8, &rr, &cc);
                touch(y, (long)j * L.YS8 + rr * L.COLS + 32 * ct + cc, 4, "MODE 3 dst", t);
            }
        }
        for (int rc = 0; rc < 8 * L.COLS; ++rc)  // the mixing's A reads: position rc of node jj
            for (int jj = 0; jj < J; ++jj) touch(y, (long)jj * L.YS8 + rc, 1, "Y read 8", t);
        std::vector<float> z((size_t)L.z_floats, 0.f);
        for (int r = 0; r < 8; ++r)
            for (int i = 0; i < J; ++i)
                for (int c = 0; c < L.COLS; c += 4) touch(z, (long)r * L.ZR + i * L.ZN + c, 4, "Z piece", t);
    }
}

int main() {
    for (const Tile& t : tiles())
        for (int ntypes = 1; ntypes <= t.J; ++ntypes) check_tile(t, ntypes);
    // pinned: MODE 2, J = 16, CT = 1 and MODE 3, J = 16
    CHECK(gl4_lds(16, 1, 2, 0, 0).bytes == 39168, "MODE 2, J = 16: %zu bytes", gl4_lds(16, 1, 2, 0, 0).bytes);
    CHECK(gl4_lds(16, 3, 3, 0, 0).bytes == 52992, "MODE 3, J = 16: %zu bytes", gl4_lds(16, 3, 3, 0, 0).bytes);
    static_assert(gl4_lds(21, 1, 2, 2, 0).bytes <= kLdsDefault, "k_gl4_pair: default dynamic LDS");
    printf("gl4 lds layout ok (%ld layouts, %ld offsets)\n", n_layouts, n_offsets);
    return 0;
}
