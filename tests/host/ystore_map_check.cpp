// Stand-alone host check of the split route's Y address map (csrc/sd_ystore_map.h), built with
// -fsanitize=address,undefined by tests/test_ystore_map_host.py.  The GEMM phase (k_gl4t, k_gl4y)
// stores a 32 x 32 tile straight from its swapped-operand MFMA accumulators: lane (l32, h), store
// g = 0..3 writes the 16-B piece of row l32, columns 8 g + 4 h .. + 3.  Checked here:
//   * the 64 lanes x 4 stores of a tile hit each of its 1,024 floats exactly once, with the value
//     the accumulator register 4 g + e of that lane holds (row l32, column 8 g + 4 h + e);
//   * the bytes of one store instruction (64 lanes, one g) are one contiguous, KiB-aligned KiB of
//     the 4-KiB scratch block, lane l32 + 32 h at byte 32 l32 + 16 h of it;
//   * the mixing phase's slab pieces (zs_slab_piece: 16- and 8-row slabs) cover their slab once and
//     consecutive pieces are consecutive in memory inside each of the four runs;
//   * the reader's zs_off maps (row, node, column) to the address the writer used, through the
//     strides the launchers pass (zs_strides), for N = 96 / 192 / 384 (the paired launch: the second
//     layer's columns start at zs_c0 = 192 of a 384-wide scratch) / 768, J = 16 / 17 / 21 and 33 /
//     257 rows -- every element of every tile written exactly once, nothing outside the scratch;
//   * the same map on a row-major destination (row stride J N): element (row, node, column).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

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

static long n_tiles = 0, n_elems = 0, n_shapes = 0;

// one tile in a 4-KiB scratch block: coverage, values, and the shape of each store instruction
static void check_tile() {
    std::vector<int> hits(1024, 0), val(1024, -1);
    for (int g = 0; g < 4; ++g) {
        std::vector<char> byte(4096, 0);
        for (int lane = 0; lane < 64; ++lane) {
            const int l32 = lane & 31, h = lane >> 5;
            const int64_t off = ystore_zs_piece_off(l32, h, g);
            CHECK(off >= 0 && off + 4 <= 1024, "piece outside the block: lane %d g %d", lane, g);
            CHECK((off & 3) == 0, "piece not 16-B aligned: lane %d g %d", lane, g);
            for (int e = 0; e < 4; ++e) {
                ++hits[off + e];
                val[off + e] = zs_blk_off(l32, ystore_col(g, h) + e);  // where the reader looks for (row, column)
                CHECK(off == 256 * g + 8 * l32 + 4 * h, "lane %d is not at byte 32 l32 + 16 h of its KiB", lane);
                for (int b = 0; b < 4; ++b) byte[(off + e) * 4 + b] = 1;
            }
        }
        // the instruction's bytes: one maximal run, the g-th KiB of the block
        int runs = 0;
        for (int i = 0; i < 4096;) {
            if (!byte[i]) {
                ++i;
                continue;
            }
            int k = i;
            while (k < 4096 && byte[k]) ++k;
            CHECK(k - i == 1024 && i == 1024 * g, "store %d: run of %d bytes at %d", g, k - i, i);
            ++runs;
            i = k;
        }
        CHECK(runs == 1, "store %d: %d runs", g, runs);
    }
    for (int i = 0; i < 1024; ++i) {
        CHECK(hits[i] == 1, "float %d written %d times", i, hits[i]);
        CHECK(val[i] == i, "float %d: the writer's element is read back from float %d", i, val[i]);
    }
    // the readers' slab pieces
    const int Rs[] = {16, 8};
    for (int R : Rs)
        for (int r0 = 0; r0 < 32; r0 += R) {
            std::vector<int> seen(1024, 0);
            int64_t prev = -1;
            for (int t = 0; t < 8 * R; ++t) {
                int r, c;
                zs_slab_piece(t, R, &r, &c);
                CHECK(r >= 0 && r < R && c >= 0 && c < 32 && c % 4 == 0, "slab piece %d of %d rows", t, R);
                const int64_t off = zs_blk_off(r0 + r, c);
                if (t % (2 * R)) CHECK(off == prev + 4, "slab piece %d of %d rows is not behind piece %d", t, R, t - 1);
                prev = off;
                for (int e = 0; e < 4; ++e) ++seen[zs_blk_off(r0 + r, c + e)];
            }
            for (int r = 0; r < 32; ++r)
                for (int c = 0; c < 32; ++c)
                    CHECK(seen[zs_blk_off(r, c)] == (r >= r0 && r < r0 + R ? 1 : 0), "slab rows %d .. of %d: (%d, %d)", r0, R, r, c);
        }
}

// writer (strides + piece map) against the reader's zs_off over a whole scratch
static void check_scratch(int J, int N, int64_t rows) {
    const int64_t ntile_r = (rows + 31) / 32;
    const int64_t total = ntile_r * 32 * J * N;
    const ZsStrides st = zs_strides(J, N);
    std::vector<int64_t> who(total, -1);  // the (row, node, column) id written to each float
    for (int64_t tr = 0; tr < ntile_r; ++tr)
        for (int j = 0; j < J; ++j)
            for (int t = 0; t < N / 32; ++t) {
                const int64_t base = tr * st.y_ts + j * st.y_js + t * st.y_cs;
                for (int lane = 0; lane < 64; ++lane)
                    for (int g = 0; g < 4; ++g)
                        for (int e = 0; e < 4; ++e) {
                            const int l32 = lane & 31, h = lane >> 5;
                            const int64_t a = base + ystore_zs_piece_off(l32, h, g) + e;
                            CHECK(a >= 0 && a < total, "store outside the scratch: J %d N %d tile %lld", J, N, (long long)tr);
                            CHECK(who[a] == -1, "float %lld written twice", (long long)a);
                            who[a] = ((tr * 32 + l32) * J + j) * N + t * 32 + ystore_col(g, h) + e;
                        }
                ++n_tiles;
            }
    for (int64_t row = 0; row < ntile_r * 32; ++row)
        for (int j = 0; j < J; ++j)
            for (int n = 0; n < N; ++n) {
                const int64_t a = zs_off(row, j, n, J, N);
                CHECK(a >= 0 && a < total, "zs_off outside the scratch");
                CHECK(who[a] == (row * J + j) * N + n, "zs_off(%lld, %d, %d) J %d N %d reads another element", (long long)row, j,
                      n, J, N);
                ++n_elems;
            }
    // the paired launch: layer b of two N / 2-wide layers reads column zs_c0 + c of the wide scratch
    if (N == 384)
        for (int c = 0; c < 192; c += 37) CHECK(who[zs_off(33, J - 1, 192 + c, J, N)] == ((int64_t)33 * J + J - 1) * N + 192 + c, "zs_c0");
    ++n_shapes;
}

// the same piece map on row-major z (rows, J, N), row stride J N, y_js = N, y_cs = 32, y_ts = 32 rows
static void check_rowmajor(int J, int N, int64_t rows) {
    const int64_t rs = (int64_t)J * N, total = rows * rs;
    std::vector<int> hits(total, 0);
    for (int64_t tr = 0; tr < (rows + 31) / 32; ++tr)
        for (int j = 0; j < J; ++j)
            for (int t = 0; t < (N + 31) / 32; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int g = 0; g < 4; ++g) {
                        const int l32 = lane & 31, h = lane >> 5;
                        const int64_t row = tr * 32 + l32;
                        const int col = t * 32 + ystore_col(g, h);
                        if (row >= rows || col >= N) continue;  // the kernels' guards (N % 4 == 0: whole pieces)
                        const int64_t a = tr * 32 * rs + (int64_t)j * N + t * 32 + ystore_rm_piece_off(l32, h, g, rs);
                        CHECK(a == (row * J + j) * N + col && a + 4 <= total, "row-major piece");
                        for (int e = 0; e < 4; ++e) ++hits[a + e];
                    }
    for (int64_t i = 0; i < total; ++i) CHECK(hits[i] == 1, "row-major float %lld written %d times", (long long)i, hits[i]);
    ++n_shapes;
}

int main() {
    check_tile();
    const int Js[] = {16, 17, 21}, Ns[] = {96, 192, 384, 768};
    const int64_t Rs[] = {33, 257};
    for (int J : Js)
        for (int N : Ns)
            for (int64_t rows : Rs) check_scratch(J, N, rows);
    check_rowmajor(51, 192, 33);
    check_rowmajor(33, 100, 67);  // N % 32 != 0, N % 4 == 0: the last tile's pieces past N are dropped
    printf("ystore map ok (%ld tiles, %ld elements, %ld shapes)\n", n_tiles, n_elems, n_shapes);
    return 0;
}
