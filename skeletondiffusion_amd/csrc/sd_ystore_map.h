// Address map of the split route's Y: where the GEMM phase (k_gl4t, k_gl4y) stores a 32 x 32 tile
// straight from its MFMA accumulators, and where the mixing phase (k_gl4 MODE 2 / 3, k_gl4_pair)
// reads it back.  Plain C++: tests/host/ystore_map_check.cpp includes this header and checks the
// writer against the reader on the host.
//
// The GEMM phase runs v_mfma_f32_32x32x16 with the weight fragment as A and the x fragment as B, so
// the accumulator tile is Y^T: lane (l32 = lane & 31, h = lane >> 5) holds batch row l32 and, in
// register r = 4 g + e (g = 0..3, e = 0..3), column 8 g + 4 h + e of the tile.  Registers 4 g ..
// 4 g + 3 are four consecutive columns of one row: one 16-B store, four per tile and lane.
//
// The scratch p.zs is [row tile][32-column tile][node] blocks of 4 KiB, and a block is
// [g 0..3][32 rows][8 columns]: the 64 lanes of store g write one contiguous KiB (lane l32 + 32 h at
// float 8 l32 + 4 h of it) -- whole 128-B lines per instruction.  (Rows of 32 columns, the layout
// before, made every store instruction write 32 B to each of 32 lines: config 2 measured 3.5 %
// slower than the LDS-transposed tail)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_YS_HD __host__ __device__ __forceinline__
#else
#define SD_YS_HD inline
#endif

namespace sd {

// first column (of the tile's 32) of the 16-B piece that lane half h stores with store g
SD_YS_HD constexpr int ystore_col(int g, int h) { return 8 * g + 4 * h; }

// float offset of that piece for the lane's row l32 ...
// ... inside a 4-KiB scratch block
SD_YS_HD constexpr int ystore_zs_piece_off(int l32, int h, int g) { return g * 256 + l32 * 8 + 4 * h; }
// ... inside a row-major tile with row stride y_rs (the J > 21 path's z)
SD_YS_HD int64_t ystore_rm_piece_off(int l32, int h, int g, int64_t y_rs) { return (int64_t)l32 * y_rs + ystore_col(g, h); }

// float offset of (row r, column c) of a tile inside its 4-KiB scratch block
SD_YS_HD int zs_blk_off(int r, int c) { return ((c >> 3) << 8) + (r << 3) + (c & 7); }

// zs element (row, node j, column n) of the split route's scratch
SD_YS_HD int64_t zs_off(int64_t row, int j, int n, int J, int N) {
    return ((((row >> 5) * (N >> 5) + (n >> 5)) * J + j) << 10) + zs_blk_off((int)(row & 31), n & 31);
}

// The mixing phase loads a slab -- rows r0 .. r0 + R - 1 (R = 16 or 8) of one block -- as 8 R / 4
// 16-B pieces, piece t by thread index: consecutive t must be consecutive in memory, so t walks
// g, then the slab's rows, then the two pieces of a row: four runs of 32 R bytes.
SD_YS_HD void zs_slab_piece(int t, int R, int* r, int* c) {
    *c = (t / (2 * R)) * 8 + (t & 1) * 4;
    *r = (t % (2 * R)) >> 1;
}

// the block strides the GEMM phase is given for that scratch: block (row tile tr, node j, column tile
// t) at y + tr y_ts + j y_js + t y_cs
struct ZsStrides {
    int64_t y_js, y_ts, y_cs;
};
SD_YS_HD ZsStrides zs_strides(int J, int N) { return ZsStrides{1024, (int64_t)(N / 32) * J * 1024, (int64_t)J * 1024}; }

}  // namespace sd
