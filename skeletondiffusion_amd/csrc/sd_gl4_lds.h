// Dynamic LDS of a v4 graph-linear tile (sd_graph_linear_v4.hip: k_gl4, k_gl4m, k_gl4_pair): the one
// statement of its layout, read by the kernels (strides, region origins) and their launchers (bytes).
// Plain C++: tests/host/gl4_lds_check.cpp checks the regions on the host.
// A tile is J nodes x 32 CT columns; MODE 0 / 1 the one-kernel tile / to_qkv + attention tile (CT = 3:
// a head's q | k | v), 2 / 3 the split route's mixing / attention phase.  In floats from the start:
//   [0, stage_h)  two weight stages of stage_h halves each (MODE 0 / 1: the K loop)
//   [sY, ...)     the Y slab, aliasing the stages after the K loop.  MODE 0 / 2: 16 rows, node j at j YS,
//                 row r at r YR (+4: 4x4 blocks read conflict-free; +16 per node: bank shift).
//                 MODE 1 / 3: 8 rows, node j at j YS8 (+16: bank shift), row r at r COLS
//   [sZ, ...)     MODE 1 / 3: 8 rows of mixed q | k | v, row r at r ZR, node i at i ZN (+4: bank shift);
//                 MODE 1 behind Y, MODE 3 over Y: max(Y, Z) is 52 KB at J = 16, two workgroups per CU
//   [sG, + J J)   G-hat, behind max(stages, Y + Z);  [sF, + 2 COLS)  FiLM (scale + 1 | shift)
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)  // (as sd_gl4_args.h, which a host check cannot include: it needs the HIP headers)
#define SD_HD __host__ __device__ __forceinline__
#elif !defined(SD_HD)
#define SD_HD inline
#endif

namespace sd {

struct Gl4Lds {
    int COLS;          // 32 CT
    int YR, YS;        // MODE 0 / 2: floats per Y row, per node of a 16-row slab
    int YS8;           // MODE 1 / 3: floats per node of an 8-row slab
    int ZN, ZR;        // MODE 1 / 3: floats per node of a Z row, per Z row
    int tile_h;        // halves of one 32-column weight tile per k chunk: hi (half / bf16 mode) or hi | lo
    int stage_h;       // halves per weight stage (0: no K loop)
    int sY, sZ, sG, sF;  // region origins (sZ: -1 without attention)
    int y_floats, z_floats;
    size_t bytes;
};

SD_HD constexpr Gl4Lds gl4_lds(int J, int CT, int MODE, int PREC, int ntypes) {
    Gl4Lds L{};
    const bool att = MODE == 1 || MODE == 3;
    L.COLS = 32 * CT;
    L.YR = L.COLS + 4;
    L.YS = 16 * L.YR + 16;
    L.YS8 = 8 * L.COLS + 16;
    L.ZN = 100;
    L.ZR = J * L.ZN;
    L.tile_h = PREC ? 512 : 1024;
    L.stage_h = MODE < 2 ? ntypes * CT * L.tile_h : 0;
    const int wfl = L.stage_h;  // two stages of halves = stage_h floats
    L.y_floats = att ? J * L.YS8 : J * L.YS;
    L.z_floats = att ? 8 * L.ZR : 0;
    L.sY = 0;
    L.sZ = MODE == 3 ? 0 : MODE == 1 ? L.y_floats : -1;
    const int yfl = MODE == 3 ? (L.y_floats > L.z_floats ? L.y_floats : L.z_floats) : L.y_floats + L.z_floats;
    L.sG = wfl > yfl ? wfl : yfl;
    L.sF = L.sG + J * J;
    L.bytes = (size_t)(L.sF + 2 * L.COLS) * sizeof(float);
    return L;
}

}  // namespace sd
