// Stand-alone host check of the split route's launch arguments, built with
// -fsanitize=address,undefined by tests/test_launch_args_host.py.  It includes the header the kernels
// and their launchers share (csrc/sd_gl4_args.h) and checks on the host:
//   * fast_divmod against the hardware's / and % (every divisor the grids use, edge dividends);
//   * decode_unit + xcd_remap against a plain 64-bit restatement of the arithmetic the kernels used
//     (u % ncg, (u / ncg) / nrg, (u / ncg) % nrg; u % ntc, (u / ntc) % J, (u / ntc) / J) for every
//     workgroup of the grids J in {16, 17, 21} x row tiles in {1, 2, 8, 9, 33, 41} x column groups in
//     {1, 2, 4, 8} x RT in {1, 2};
//   * that xcd_remap is a bijection of [0, grid) also where the grid is no multiple of 8, and keeps
//     the units of one XCD contiguous;
//   * that the packers fill every argument block with what the GLArgs fields imply.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_gl4_args.h"

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

static long n_div = 0, n_units = 0, n_grids = 0;

static void check_divisor(uint32_t d) {
    const FastDiv f = make_fastdiv(d);
    const uint32_t us[] = {0u, 1u, 2u, d - 1, d, d + 1, 2 * d - 1, 2 * d, 3 * d + 1, 65535u, 65536u, 1u << 24, (1u << 24) + 1,
                           0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu / d * d, 0xFFFFFFFFu / d * d - 1};
    for (uint32_t u : us) {
        uint32_t q, r;
        fast_divmod(u, f, q, r);
        CHECK(q == u / d && r == u % d, "fast_divmod(%u, %u) = (%u, %u)", u, d, q, r);
        ++n_div;
    }
    uint32_t x = 2463534242u ^ d;
    for (int i = 0; i < 2000; ++i) {  // xorshift dividends over the whole 32-bit range
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        uint32_t q, r;
        fast_divmod(x, f, q, r);
        CHECK(q == x / d && r == x % d, "fast_divmod(%u, %u) = (%u, %u)", x, d, q, r);
        ++n_div;
    }
}

// the arithmetic k_gl4t used before (64-bit / and %), restated
static void ref_gl4t(int64_t block, int64_t nwg, int64_t ncg, int64_t nrg, int64_t* j, int64_t* rgi, int64_t* cg, int64_t* u_out) {
    const int64_t xcd = block & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int64_t u = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (block >> 3);
    *cg = u % ncg;
    *j = (u / ncg) / nrg;
    *rgi = (u / ncg) % nrg;
    *u_out = u;
}

static void check_gl4t_grid(int J, int64_t ntile_r, int ncg, int RT) {
    const int64_t nrg = (ntile_r + 4 * RT - 1) / (4 * RT);
    const int64_t nwg = nrg * J * ncg;
    CHECK(gl4_grid_ok(nwg), "grid %lld", (long long)nwg);
    const FastDiv da = make_fastdiv((uint32_t)ncg), db = make_fastdiv((uint32_t)nrg);
    const uint32_t q8 = (uint32_t)(nwg >> 3), r8 = (uint32_t)(nwg & 7);
    std::vector<int> seen((size_t)nwg, 0);
    std::vector<int64_t> lo8(8, -1), hi8(8, -1), cnt8(8, 0);
    for (int64_t b = 0; b < nwg; ++b) {
        int64_t j, rgi, cg, u;
        ref_gl4t(b, nwg, ncg, nrg, &j, &rgi, &cg, &u);
        const uint32_t u32 = xcd_remap((uint32_t)b, q8, r8);
        CHECK((int64_t)u32 == u, "remap block %lld of %lld: %u vs %lld", (long long)b, (long long)nwg, u32, (long long)u);
        CHECK(u >= 0 && u < nwg, "unit %lld outside the grid %lld", (long long)u, (long long)nwg);
        CHECK(seen[(size_t)u]++ == 0, "unit %lld taken twice (grid %lld)", (long long)u, (long long)nwg);
        const Unit3 un = decode_unit(u32, da, db);
        CHECK(un.lo == cg && un.mid == rgi && un.hi == j, "decode unit %lld (J %d, tiles %lld, ncg %d, RT %d)", (long long)u, J,
              (long long)ntile_r, ncg, RT);
        CHECK(j < J && rgi < nrg && cg < ncg, "unit %lld out of range", (long long)u);
        const int x = (int)(b & 7);
        if (lo8[x] < 0 || u < lo8[x]) lo8[x] = u;
        if (u > hi8[x]) hi8[x] = u;
        ++cnt8[x];
        ++n_units;
    }
    for (int x = 0; x < 8; ++x)  // one XCD's units are a contiguous run
        CHECK(cnt8[x] == 0 || hi8[x] - lo8[x] + 1 == cnt8[x], "XCD %d: units not contiguous (grid %lld)", x, (long long)nwg);
    ++n_grids;
}

static void check_gl4y_grid(int J, int64_t ntile_r, int ntc) {
    const int64_t units = ntile_r * J * ntc, nblk = (units + 3) / 4;
    CHECK(gl4_grid_ok(units + 3), "grid");
    const FastDiv da = make_fastdiv((uint32_t)ntc), db = make_fastdiv((uint32_t)J);
    for (int64_t b = 0; b < nblk; ++b)
        for (int wave = 0; wave < 4; ++wave) {
            const int64_t u = b * 4 + wave;  // the last block's spare waves decode to row tile >= ntile_r
            const int64_t tc = u % ntc, rj = u / ntc, j = rj % J, tr = rj / J;
            const Unit3 un = decode_unit((uint32_t)b * 4u + (uint32_t)wave, da, db);
            CHECK(un.lo == tc && un.mid == j && un.hi == tr, "k_gl4y unit %lld", (long long)u);
            CHECK((u < units) == (tr < ntile_r), "k_gl4y live-unit test, unit %lld", (long long)u);
            ++n_units;
        }
    ++n_grids;
}

// mixing phase: block -> (row tile, column tile, slab)
static void check_mix_grid(int64_t ntile_r, int ntc, int slabs) {
    const FastDiv f = make_fastdiv((uint32_t)ntc);
    const int sh = slabs == 2 ? 1 : 2;
    for (int64_t b = 0; b < ntile_r * ntc * slabs; ++b) {
        const int L = (int)(b >> sh);
        uint32_t q, r;
        fast_divmod((uint32_t)L, f, q, r);
        CHECK((int)r == L % ntc && (int)q == L / ntc, "mixing block %lld", (long long)b);
        ++n_units;
    }
    ++n_grids;
}

static void check_pair_grid(int64_t ntile_r, int nta, int ntb) {
    const FastDiv f = make_fastdiv((uint32_t)(nta + ntb));
    for (int64_t b = 0; b < ntile_r * (nta + ntb) * 2; ++b) {
        const int L = (int)(b >> 1), slab = (int)(b & 1);
        const int pt = L % (nta + ntb), tr = L / (nta + ntb);
        const int want = pt < nta ? ((tr * nta + pt) << 1) | slab : ((tr * ntb + pt - nta) << 1) | slab;
        uint32_t q, r;
        fast_divmod((uint32_t)(b >> 1), f, q, r);
        const uint32_t got = r < (uint32_t)nta ? ((q * nta + r) << 1) | (uint32_t)slab : ((q * ntb + r - nta) << 1) | (uint32_t)slab;
        CHECK((int)got == want && (int)r == pt, "pair block %lld", (long long)b);
        ++n_units;
    }
    ++n_grids;
}

static GLArgs layer(int J, int N, int ntypes, int pair_n) {
    static float buf[64];
    static _Float16 wbuf[8];
    static unsigned st;
    GLArgs a{};
    a.x1 = buf + 1; a.x1_rs = 7 * 96; a.K1 = 192; a.x1_div = 50; a.x1_row0 = 17;
    a.x2 = buf + 2; a.x2_rs = J * 192; a.K2 = 192;
    a.W = buf + 3; a.bias = buf + 4; a.G = buf + 5; a.film = buf + 6; a.ln_w = buf + 7; a.ln_b = buf + 8;
    a.res = buf + 9; a.res_rs = (int64_t)J * N; a.out = buf + 10; a.out_rs = (int64_t)J * N + 4;
    a.B = 3217; a.N = N; a.J = J; a.act = 1; a.ntypes = ntypes;
    for (int j = 0; j < J; ++j) {
        a.ntype[j] = (j * 7 + 3) % ntypes;
        a.wrow[j] = a.ntype[j] * N;
    }
    a.wsp = wbuf; a.wsp_nct = 24; a.wsp_unscale = 0.125f; a.prec = 0;
    a.attn_heads = 8; a.attn_scale = 0.1767767f;
    a.x1_blk = 0; a.x2_blk = 1; a.res_blk = 1; a.out_blk = 1;
    a.zs = buf + 11; a.zs_cap = 1 << 20; a.status = &st;
    a.pair_n = pair_n; a.W2 = buf + 12; a.wsp_unscale2 = 0.25f;
    return a;
}

static void check_packers() {
    for (int J : {16, 17, 21, 51}) {
        const int ntypes = J == 16 ? 10 : J == 51 ? 21 : 13;
        GLArgs a = layer(J, 192, ntypes, 0);
        GL4GArgs g;
        memset(&g, 0xAB, sizeof g);
        const int64_t ntile_r = (a.B + 31) / 32;
        float* y = a.zs;
        CHECK(pack_gl4g(a, ntile_r, y, 32, 1024, (int64_t)(a.N / 32) * J * 1024, (int64_t)J * 1024, 6, (uint32_t)J, 1234567u, &g), "pack");
        CHECK(g.x1 == a.x1 && g.x2 == a.x2 && g.wsp == a.wsp && g.bias == a.bias && g.W == a.W && g.W2 == a.W2 &&
                  g.status == a.status && g.y == y, "pointers");
        CHECK(g.x1_rs == a.x1_rs && g.x2_rs == a.x2_rs && g.x1_row0 == a.x1_row0 && g.B == a.B && g.ntile_r == ntile_r, "rows");
        CHECK(g.y_rs == 32 && g.y_js == 1024 && g.y_ts == (int64_t)(a.N / 32) * J * 1024 && g.y_cs == J * 1024, "Y strides");
        CHECK(g.K1 == a.K1 && g.K2 == a.K2 && g.x1_div == a.x1_div && g.N == a.N && g.J == a.J && g.pair_n == a.pair_n &&
                  g.wsp_nct == a.wsp_nct && g.wsp_unscale == a.wsp_unscale && g.wsp_unscale2 == a.wsp_unscale2, "scalars");
        CHECK(g.da.d == 6 && g.db.d == (uint32_t)J && g.q8 == 1234567u / 8 && g.r8 == 1234567u % 8, "grid factors");
        CHECK(g.x1_blk == 0 && g.x2_blk == 1 && g.x1_bf16 == 0 && g.x2_bf16 == 0, "layout flags");
        for (int j = 0; j < J; ++j) {
            const int t = gl4_node_type(g, j);
            // the offsets the kernels form from the type: the bias / f32 weight row, the split-weight slice
            CHECK(t == a.ntype[j] && t * g.N == a.wrow[j], "node %d: type %d vs %d, row %d vs %d", j, t, a.ntype[j], t * g.N, a.wrow[j]);
        }
        for (int j = J; j < kMaxNodes; ++j) CHECK(gl4_node_type(g, j) == 0, "unused node slot %d", j);
        for (size_t i = 0; i < sizeof g.line_pad_ / sizeof g.line_pad_[0]; ++i) CHECK(g.line_pad_[i] == 0, "padding");
        // a paired launch: N = 2 pair_n, the second layer's row is type * pair_n = wrow >> 1
        GLArgs pr = layer(J, 384, ntypes, 192);
        CHECK(pack_gl4g(pr, ntile_r, y, 32, 1024, 12ll * J * 1024, (int64_t)J * 1024, 4, 13, 999u, &g), "pack pair");
        for (int j = 0; j < J; ++j) CHECK(gl4_node_type(g, j) * g.pair_n == pr.wrow[j] >> 1, "pair row of node %d", j);
        // refusals: a type that needs more than a byte, a wrow that is not type * N, strides over 32 bits
        GLArgs bad = a;
        bad.ntype[3] = 256; bad.wrow[3] = 256 * bad.N;
        CHECK(!pack_gl4g(bad, ntile_r, y, 32, 1024, 1, 1, 6, 16, 8, &g), "type 256 accepted");
        bad = a;
        bad.wrow[5] += 1;
        CHECK(!pack_gl4g(bad, ntile_r, y, 32, 1024, 1, 1, 6, 16, 8, &g), "foreign wrow accepted");
        CHECK(!pack_gl4g(a, ntile_r, y, (int64_t)1 << 31, 1024, 1, 1, 6, 16, 8, &g), "64-bit row stride accepted");
        CHECK(!pack_gl4g(a, ntile_r, y, 32, 1024, 1, 1, 0, 16, 8, &g), "zero divisor accepted");

        GL4MArgs m;
        memset(&m, 0xCD, sizeof m);
        GLArgs b = layer(J, 192, ntypes, 0);
        b.zs_n = 384; b.zs_c0 = 192; b.res_bf16 = 1;
        CHECK(pack_gl4m(b, 6, &m), "pack mix");
        CHECK(m.zs == b.zs && m.G == b.G && m.film == b.film && m.ln_w == b.ln_w && m.ln_b == b.ln_b && m.res == b.res && m.out == b.out,
              "mix pointers");
        CHECK(m.B == b.B && m.res_rs == b.res_rs && m.out_rs == b.out_rs && m.N == b.N && m.zs_n == 384 && m.zs_c0 == 192 &&
                  m.act == b.act && m.attn_heads == b.attn_heads && m.attn_scale == b.attn_scale && m.ntc.d == 6, "mix scalars");
        CHECK(m.res_blk == 1 && m.out_blk == 1 && m.res_bf16 == 1 && m.out_bf16 == 0, "mix flags");
        for (size_t i = 0; i < sizeof m.line_pad_ / sizeof m.line_pad_[0]; ++i) CHECK(m.line_pad_[i] == 0, "mix padding");
        b.zs_n = 0;
        CHECK(pack_gl4m(b, 6, &m) && m.zs_n == b.N, "scratch width of an unpaired layer");
        CHECK(!pack_gl4m(b, 0, &m), "zero column tiles accepted");

        GL4PairArgs pp;
        GLArgs pa = layer(J, 192, ntypes, 0), pb = layer(J, 96, ntypes, 0);
        pa.zs_n = pb.zs_n = 288; pb.zs_c0 = 192; pb.act = 0;
        CHECK(pack_gl4_pair(pa, pb, &pp), "pack pair mix");
        CHECK(pp.nta == 6 && pp.nt.d == 9 && pp.a.ntc.d == 6 && pp.b.ntc.d == 3 && pp.a.zs_c0 == 0 && pp.b.zs_c0 == 192 &&
                  pp.a.act == 1 && pp.b.act == 0 && pp.a.zs_n == 288 && pp.b.zs_n == 288, "pair fields");
        pb.N = 100;
        CHECK(!pack_gl4_pair(pa, pb, &pp), "N = 100 accepted");
    }
    CHECK(!gl4_grid_ok(0) && gl4_grid_ok(1) && gl4_grid_ok(((int64_t)1 << 31) - 1) && !gl4_grid_ok((int64_t)1 << 31), "grid bound");
    CHECK(sizeof(GL4GArgs) % 64 == 0 && sizeof(GL4MArgs) % 64 == 0 && sizeof(GL4PairArgs) % 64 == 0, "whole lines");
}

int main() {
    for (uint32_t d = 1; d <= 4100; ++d) check_divisor(d);
    for (uint32_t d : {65535u, 65536u, 65537u, 1u << 20, (1u << 24) - 1, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu})
        check_divisor(d);
    for (int J : {16, 17, 21})
        for (int64_t tiles : {1, 2, 8, 9, 33, 41})
            for (int ncg : {1, 2, 4, 8}) {
                for (int RT : {1, 2}) check_gl4t_grid(J, tiles, ncg, RT);
                check_gl4y_grid(J, tiles, ncg);
                check_gl4y_grid(J, tiles, 3 * ncg);
                check_mix_grid(tiles, 3 * ncg, 2);
                check_mix_grid(tiles, ncg, 4);
                check_pair_grid(tiles, 3 * ncg, 6);
            }
    check_gl4t_grid(51, 101, 3, 1);  // the row-major GEMM phase of J > 21
    check_packers();
    printf("launch decode ok (%ld divisions, %ld units, %ld grids)\n", n_div, n_units, n_grids);
    return 0;
}
