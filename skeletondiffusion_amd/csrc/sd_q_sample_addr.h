// Address arithmetic, the row -> (sequence, copy) -> Philox-row map and the per-quad arithmetic of the
// grouped forward process (sd_q_sample.hip), as host + device functions: the kernel takes every global
// offset, LDS index, loop bound and sum from here, and so does the stand-alone host emulation
// (tests/host/q_sample_emulation.cpp), which walks every workgroup x thread x load / store with the
// same functions and checks each against the size of the buffer it goes to.
//
// One workgroup per output row o.  Without `sel` the launch has nseq k rows in repeat_interleave order,
// o = s k + copy; with `sel` it has nseq rows, o = s and copy = clamp(sel[s], 0, k - 1).  Either way
// the row's draws are keyed by its global row in the full launch, row0 + s k + copy, and a supplied
// noise_in (nseq k, J, D) is read at row s k + copy: a `sel` launch returns the bits of the same rows of
// the full launch.
// Philox quad map (key = seed, row as above, step; philox_at in sd_philox.h): quad q of a row holds the
// elements 4 q .. 4 q + 3 of its J D values, (x, y) -> box_muller -> elements 0 and 1, (z, w) -> 2 and 3:
// the sampler's order (k_noise_fill), oracle.philox_normal(seed, rows, step, J D).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_QHD __host__ __device__ inline
#else
#define SD_QHD inline
#endif

namespace sd {
namespace qsample {

constexpr int kThreads = 256;  // threads of every workgroup here
constexpr int kMaxJoints = 64, kMinDim = 4, kMaxDim = 256;

// workgroups (= output rows) of a launch
SD_QHD int64_t out_rows(int64_t nseq, int k, bool has_sel) { return has_sel ? nseq : nseq * k; }

struct RowMap {
    int64_t seq;         // sequence: the row of x0 and t
    int copy;            // which of the sequence's k copies
    int64_t noise_row;   // row of noise_in / of the full launch: seq k + copy
    uint64_t philox_row; // row0 + noise_row
};

// a timestep / a selection outside its range is clamped, so the table and noise reads stay in bounds
SD_QHD int clamp_t(int64_t t, int T) { return t < 0 ? 0 : (t > T - 1 ? T - 1 : (int)t); }
SD_QHD int clamp_sel(int64_t c, int k) { return c < 0 ? 0 : (c > k - 1 ? k - 1 : (int)c); }

// output row o of a launch; sel_value = sel[o] (read only when has_sel)
SD_QHD RowMap row_map(int64_t o, int k, bool has_sel, int64_t sel_value, int64_t row0) {
    RowMap m;
    m.seq = has_sel ? o : o / k;
    m.copy = has_sel ? clamp_sel(sel_value, k) : (int)(o - m.seq * k);
    m.noise_row = m.seq * k + m.copy;
    m.philox_row = (uint64_t)(row0 + m.noise_row);
    return m;
}

// ---- a row's J D values as quads ------------------------------------------------------------------
SD_QHD int quads(int J, int D) { return J * (D >> 2); }
SD_QHD int quad_elem(int q) { return 4 * q; }                      // first element of quad q (also its LDS index)
// element e of row r of a (rows, J, D) tensor
SD_QHD int64_t row_elem(int64_t r, int J, int D, int e) { return r * (int64_t)(J * D) + e; }
// the mixing pass: item q in [0, quads) is (joint i, feature quad) of the output row, the same split
SD_QHD int item_joint(int q, int D) { return q / (D >> 2); }
SD_QHD int item_d0(int q, int D) { return 4 * (q % (D >> 2)); }
// row i of M[t] in M (T, J, J)
SD_QHD int64_t m_row(int t, int J, int i) { return ((int64_t)t * J + i) * J; }
// floats of LDS a workgroup needs: the row's noise when it is mixed across joints, nothing otherwise
SD_QHD size_t lds_floats(int J, int D, bool mixing) { return mixing ? (size_t)J * D : 0; }

// ---- arithmetic (f32; one fused multiply-add per product after the first) -------------------------
// out[c] = a x0[c] + sum_j Mrow[j] eps[j D + d0 + c], j ascending
SD_QHD void mix_quad(float a, const float* x0q, const float* Mrow, const float* eps, int J, int D, int d0, float* out) {
    float acc[4];
    for (int c = 0; c < 4; ++c) acc[c] = a * x0q[c];
    for (int j = 0; j < J; ++j) {
        const float m = Mrow[j];
        const float* e = eps + (size_t)j * D + d0;
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(m, e[c], acc[c]);
    }
    for (int c = 0; c < 4; ++c) out[c] = acc[c];
}
// out[c] = a x0[c] + b eps[c]   (the isotropic sibling)
SD_QHD void iso_quad(float a, const float* x0q, float b, const float* eq, float* out) {
    for (int c = 0; c < 4; ++c) out[c] = fmaf(b, eq[c], a * x0q[c]);
}

}  // namespace qsample
}  // namespace sd
