// Index arithmetic, orderings and the greedy step of the diversity ranking (sd_rank.hip),
// as host/device code: tests/host/rank_emulation.cpp walks the same functions under AddressSanitizer.
//
// A sequence's points are P_0 = its target and P_{1+s} = its sample s, N = samples + 1 of them.  The
// distance matrix (N, N) is cut into tiles of kTile x kTile; only the tile pairs ti <= tj are computed, and
// inside a diagonal tile only the entries i <= j; every entry i < j is stored at (i, j) and at (j, i).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_RANK_HD __host__ __device__ __forceinline__
#else
#define SD_RANK_HD inline
#endif

namespace sd {
namespace rank {

constexpr int kTile = 32;        // points per tile side
constexpr int kMaxPoints = 256;  // samples + 1 <= kMaxPoints: one thread of the selection per point
constexpr int kThreads = 256;
constexpr int kWave = 64;

SD_RANK_HD int tiles(int points) { return (points + kTile - 1) / kTile; }
SD_RANK_HD int tile_pairs(int points) { return tiles(points) * (tiles(points) + 1) / 2; }

// pair p in [0, tile_pairs): row-major over the upper triangle, (0,0) (0,1) .. (0,T-1) (1,1) ..
SD_RANK_HD void pair_tiles(int p, int ntiles, int* ti, int* tj) {
    int i = 0, row = ntiles;  // `row` pairs start with ti = i
    while (p >= row) {
        p -= row;
        --row;
        ++i;
    }
    *ti = i;
    *tj = i + p;
}

// element offset of point `pt` of sequence b: into target (pt == 0) or into pred (pt >= 1)
SD_RANK_HD int64_t point_offset(int64_t b, int pt, int samples, int64_t features) {
    return pt == 0 ? b * features : (b * samples + (pt - 1)) * features;
}

SD_RANK_HD int64_t dist_offset(int64_t b, int points, int i, int j) { return (b * points + i) * points + j; }

// whether the tile pair (ti, tj) computes and stores entry (i, j) (then also at (j, i) when i != j)
SD_RANK_HD bool owns(int ti, int tj, int i, int j, int points) { return i < points && j < points && (ti != tj || i <= j); }

SD_RANK_HD bool is_nan(float v) { return v != v; }

// Candidates are (value, index) with index < 0 = none.  The arg-max order: a larger value wins, NaN ranks
// below every number, equal values (and two NaNs) go to the lower index.
SD_RANK_HD bool better_max(float va, int ia, float vb, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    const bool na = is_nan(va), nb = is_nan(vb);
    if (na || nb) return na && nb ? ia < ib : nb;
    if (va != vb) return va > vb;
    return ia < ib;
}

// The arg-min order of the closest sample: a smaller value wins, NaN ranks above every number, ties to
// the lower index.
SD_RANK_HD bool better_min(float va, int ia, float vb, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    const bool na = is_nan(va), nb = is_nan(vb);
    if (na || nb) return na && nb ? ia < ib : nb;
    if (va != vb) return va < vb;
    return ia < ib;
}

// m_i = min(m_i, d(i, c)); NaN on either side stays (torch.minimum)
SD_RANK_HD float min_nan(float a, float b) {
    if (is_nan(a)) return a;
    if (is_nan(b)) return b;
    return b < a ? b : a;
}

// One step of the fixed reduction tree (a wave's xor butterfly with offsets 32, 16, .., 1, then the waves
// in wave order): the candidate (v, i) meets (ov, oi) and keeps the better one.  The orders are total, so
// every lane of a wave ends with the same winner.
template <bool MAX>
SD_RANK_HD void meet(float* v, int* i, float ov, int oi) {
    if (MAX ? better_max(ov, oi, *v, *i) : better_min(ov, oi, *v, *i)) {
        *v = ov;
        *i = oi;
    }
}

// the waves' results, in wave order
template <bool MAX>
SD_RANK_HD void block_best(const float* wv, const int* wi, int nwaves, float* v, int* i) {
    *v = wv[0];
    *i = wi[0];
    for (int w = 1; w < nwaves; ++w) meet<MAX>(v, i, wv[w], wi[w]);
}

// the matrix of [anchor; samples] read from the matrix of [target; samples]: row / column 0 are the anchor's
SD_RANK_HD int anchored(int i, int anchor) { return i == 0 ? anchor : i; }

// ---- phase 1: one 64-thread workgroup per tile pair --------------------------------------------------------
constexpr int kDistThreads = 64;
constexpr int kKC = 32;        // features per chunk (sd_cdist's summation order)
constexpr int kKQ = kKC / 4;   // k quads (float4 of four consecutive features) per chunk
constexpr int kLd = kTile + 2; // float4 slots per k quad (padded: the k quads of a row fall on different banks)
constexpr int kQ = kTile * kKQ / kDistThreads;  // quads a thread loads per operand and chunk: 4
constexpr int kOut = 4;        // a thread's outputs: kOut x kOut

// loader role: quad q of thread tid is tile row load_row(tid, q), k quad load_kq(tid)
SD_RANK_HD int load_row(int tid, int q) { return (tid >> 3) + 8 * q; }
SD_RANK_HD int load_kq(int tid) { return tid & 7; }
// LDS slot of k quad kq of tile row r in the row operand, of tile column c in the column operand
SD_RANK_HD int a_slot(int kq, int r) { return kq * kLd + r; }
SD_RANK_HD int b_slot(int kq, int c) { return kq * kLd + (c & 3) * 8 + (c >> 2); }
// compute role: thread tid owns tile rows out_row(tid, i) and tile columns out_col(tid, j), i, j < kOut
SD_RANK_HD int out_row(int tid, int i) { return (tid >> 3) + 8 * i; }
SD_RANK_HD int out_col(int tid, int j) { return 4 * (tid & 7) + j; }
// k quads of chunk c that hold a feature
SD_RANK_HD int chunk_quads(int64_t features, int64_t c) {
    const int64_t left = (features - c * kKC + 3) / 4;
    return (int)(left < kKQ ? left : kKQ);
}

}  // namespace rank
}  // namespace sd
