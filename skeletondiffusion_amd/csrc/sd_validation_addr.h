// Address arithmetic of the validation-metric kernels (sd_validation.hip), as host + device functions:
// the kernels take every global offset, LDS index, loop bound and thread role from here, and so does
// the stand-alone host emulation (tests/host/validation_emulation.cpp), which walks every workgroup x
// thread x load / store with the same functions and checks each against the size of the buffer it
// goes to.  The limb-statistics pass stages frames exactly as the body-realism pass does, so the
// frame tile, the sample / target frame offsets and the 16-byte split are sd_realism_addr.h's own.
// Also here, because the emulation checks them against plain two-pass arithmetic: the combine step
// of the variance, the NaN-keeping maximum / minimum, and the clamp of a row's sample index.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sd_realism_addr.h"

namespace sd {
namespace validation {

using realism::frame_tile;
using realism::kMaxJoints;
using realism::kMaxLimbs;
using realism::kMaxSamples;
using realism::kThreads;
using realism::limb_index;
using realism::pred_frame;
using realism::stage_split;
using realism::target_frame;

// ---- limb statistics ---------------------------------------------------------------------------------
// per (sequence, sample, limb), planes of the (5, B * S, L) array (realism::limb_index)
constexpr int kStats = 5;
enum Stat { kVar = 0, kJitMean = 1, kJitMax = 2, kJitMin = 3, kErr = 4 };
// per (sequence, sample), over the limbs: rows of the (7, B * S) arrays
constexpr int kSampleRows = 7;
enum SampleRow { kSVarMean = 0, kSVarMax, kSVarMin, kSJitMean, kSJitMax, kSJitMin, kSErrMean };
// per sequence, over the samples: rows of the (9, B) array; row r < 7 reduces sample row r with its own
// operation (mean / max / min), rows 7 and 8 are the maximum and the minimum of kSErrMean
constexpr int kSeqRows = 9;
enum SeqRow { kQErrMax = 7, kQErrMin = 8 };
// 0 mean, 1 max, 2 min: how a sample row (over limbs) and a sequence row (over samples) reduce
SD_RHD int sample_row_op(int r) { return r == kSVarMax || r == kSJitMax ? 1 : (r == kSVarMin || r == kSJitMin ? 2 : 0); }
SD_RHD int sample_row_stat(int r) {
    return r <= kSVarMin ? kVar : (r == kSJitMean ? kJitMean : (r == kSJitMax ? kJitMax : (r == kSJitMin ? kJitMin : kErr)));
}
SD_RHD int seq_row_source(int r) { return r < kSampleRows ? r : kSErrMean; }
SD_RHD int seq_row_op(int r) { return r == kQErrMax ? 1 : (r == kQErrMin ? 2 : sample_row_op(r)); }

SD_RHD int64_t sample_index(int r, int64_t BS, int64_t w) { return (int64_t)r * BS + w; }  // (7, B * S)
SD_RHD int64_t seq_index(int r, int64_t B, int64_t b) { return (int64_t)r * B + b; }        // (9, B)
// |len_t - len_{t-1}| of limb l, step t - 1 -> t (1 <= t < T), of sample w in steps_out (B * S, T - 1, L)
SD_RHD int64_t step_index(int64_t w, int T, int t, int L, int l) { return (w * (int64_t)(T - 1) + (t - 1)) * L + l; }

// dynamic LDS of the limb pass: doubles ll[tile][L] (the sample's limb lengths) and tl[tile][L] (the
// target's), then floats frames[tile][3 J]
SD_RHD int lds_len_doubles(int J, int L) { return frame_tile(J) * L; }
SD_RHD int lds_stage_floats(int J) { return frame_tile(J) * 3 * J; }
SD_RHD size_t limb_lds_bytes(int J, int L) {
    return sizeof(double) * 2 * (size_t)lds_len_doubles(J, L) + sizeof(float) * (size_t)lds_stage_floats(J);
}

// Chan's combine step: (n, mean, m2 = sum (x - mean)^2) of a set joined with those of a disjoint set.
// The variance is never a difference of raw second moments: each tile's m2 is taken about its own mean.
SD_RHD void var_combine(double& n, double& mean, double& m2, double nb, double meanb, double m2b) {
    const double nt = n + nb, delta = meanb - mean;
    mean = mean + delta * (nb / nt);
    m2 = (m2 + m2b) + (delta * delta) * (n * nb / nt);
    n = nt;
}
// torch.max / torch.min of a running value and the next: a NaN stays
SD_RHD double max_keep_nan(double m, double x) { return (x != x || m != m) ? (m != m ? m : x) : (x > m ? x : m); }
SD_RHD double min_keep_nan(double m, double x) { return (x != x || m != m) ? (m != m ? m : x) : (x < m ? x : m); }

// ---- streaming frame error ---------------------------------------------------------------------------
// A workgroup owns kCells consecutive (frame, joint) cells of the window and walks the rows kRows at a
// time: thread tid is (row tid / kCells of the pass, lane tid % kCells).
constexpr int kCells = 16, kRows = 16;
static_assert(kCells * kRows == kThreads, "one thread per (row of the pass, cell)");
constexpr int kSpanFloats = 3 * kCells;  // floats of one row's span (its cells' coordinates are contiguous)

SD_RHD int64_t cell_count(int nframes, int J) { return (int64_t)nframes * J; }
SD_RHD int cells_of_block(int64_t cells, int64_t block) {
    const int64_t left = cells - block * kCells;
    return left < kCells ? (int)left : kCells;
}
// the sample a row takes: idx when it is a sample, else -1 (the row contributes NaN and reads no pred)
SD_RHD int sample_or_none(int64_t idx, int S) { return idx >= 0 && idx < S ? (int)idx : -1; }
// first float of cell c0 (counted from the window's first frame) of row r, sample s, in pred (R, S, T, J, 3)
SD_RHD int64_t pred_span(int64_t r, int s, int S, int T, int J, int frame0, int64_t c0) {
    return ((r * S + s) * T + frame0) * (int64_t)(3 * J) + 3 * c0;
}
// ... of row r in target (R, T, J, 3)
SD_RHD int64_t target_span(int64_t r, int T, int J, int frame0, int64_t c0) {
    return (r * T + frame0) * (int64_t)(3 * J) + 3 * c0;
}
// What lane k of a row's kCells threads copies of a span of N <= kSpanFloats floats split by
// stage_split into head / quads / tail: 16-byte load k (if k < quads) and one of the <= 6 single floats
// (element `scalar`, or -1)
SD_RHD void span_lane(int k, int N, int head, int quads, int& quad, int& scalar) {
    quad = k < quads ? k : -1;
    const int tail0 = head + 4 * quads, singles = head + (N - tail0);
    scalar = k < singles ? (k < head ? k : tail0 + (k - head)) : -1;
}
SD_RHD int lds_span(int row, int e) { return row * kSpanFloats + e; }  // float e of a pass row's staged span
SD_RHD int lds_cell(int row, int c) { return row * kCells + c; }       // the norm of (pass row, cell)

}  // namespace validation
}  // namespace sd
