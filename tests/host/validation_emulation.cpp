// Host emulation of the address arithmetic of sd_validation.hip (k_limb_stats, k_limb_reduce,
// k_frame_error): every workgroup x thread x load / store of the three kernels, with the offsets, LDS
// indices, loop bounds and thread roles of skeletondiffusion_amd/csrc/sd_validation_addr.h, the same
// functions the kernels call.  Small shapes run on real heap buffers of the exact sizes (build with
// -fsanitize=address,undefined: an access outside one aborts); large shapes check every index against the
// buffer's size arithmetically.  16-byte loads must be 16-byte aligned and stay inside the span they copy;
// a staged span must be covered exactly once.  The header's arithmetic helpers are checked as well: the
// variance combine step against a two-pass variance on near-rigid lengths, the NaN-keeping maximum /
// minimum, and the clamp of a row's sample index.
// Built and run by tests/test_validation_host.py; no GPU, nothing preloaded.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_validation_addr.h"

using namespace sd::validation;

namespace {

long long g_accesses = 0;

[[noreturn]] void die(const char* what, int64_t idx, int64_t size) {
    std::fprintf(stderr, "out of bounds: %s index %" PRId64 " size %" PRId64 "\n", what, idx, size);
    std::abort();
}

// a buffer of `size` elements of type E at a pretended byte address; `real` holds it on the heap or is empty
template <class E>
struct Buf {
    const char* name;
    int64_t size;
    uint64_t addr;  // pretended device address of element 0
    std::vector<E> real;
    Buf(const char* n, int64_t s, bool make_real, uint64_t a = 0x10000) : name(n), size(s), addr(a) {
        if (make_real) real.assign((size_t)s, E(1));
    }
    E ld(int64_t i, int width = 1) {
        if (i < 0 || i + width > size) die(name, i, size);
        if (width > 1 && (addr + sizeof(E) * (uint64_t)i) % (sizeof(E) * width)) die("misaligned vector load", i, size);
        g_accesses += width;
        E v = E(0);
        if (!real.empty())
            for (int k = 0; k < width; ++k) v += real.data()[i + k];  // a raw read: the sanitizer sees it
        return v;
    }
    void st(int64_t i, E v) {
        if (i < 0 || i >= size) die(name, i, size);
        ++g_accesses;
        if (!real.empty()) real.data()[i] = v;
    }
};

struct LimbShape {
    int64_t B;
    int S, T, J, L;
};

void joint(Buf<float>& b, int64_t base, int j) {  // the three floats of a joint
    b.ld(base + 3 * j);
    b.ld(base + 3 * j + 1);
    b.ld(base + 3 * j + 2);
}

void emulate_limb(const LimbShape& s, bool real, int phase, bool with_target) {
    const int J3 = 3 * s.J, TF = frame_tile(s.J);
    const int64_t BS = s.B * s.S;
    std::vector<int> la, lb;  // joint indices that sweep the whole range, both orders
    for (int l = 0; l < s.L; ++l) {
        la.push_back(l % 2 ? s.J - 1 - (l % s.J) : l % s.J);
        lb.push_back(l % 3 ? (l * 7) % s.J : s.J - 1);
    }
    Buf<float> pred("pred", BS * s.T * J3, real, 0x10000 + 4 * (uint64_t)phase);
    Buf<float> target("target", s.B * s.T * J3, real);
    Buf<float> limb_out("limb_out", kStats * BS * s.L, real), sample_out("sample_out", kSampleRows * BS, real),
        seq_out("seq_out", kSeqRows * s.B, real), steps("steps_out", BS * (s.T - 1) * s.L, real),
        diff("steps_diff_out", BS * (s.T - 1) * s.L, real);
    Buf<double> scratch("sample_scratch", kSampleRows * BS, real);

    // ---- k_limb_stats: grid B * S, dynamic LDS limb_lds_bytes(J, L) ----
    if (limb_lds_bytes(s.J, s.L) > 64 * 1024) die("dynamic LDS bytes", (int64_t)limb_lds_bytes(s.J, s.L), 64 * 1024);
    for (int64_t w = 0; w < BS; ++w) {
        const int64_t b = w / s.S;
        Buf<double> ll("ll (LDS)", lds_len_doubles(s.J, s.L), real), tl("tl (LDS)", lds_len_doubles(s.J, s.L), real);
        Buf<float> fr("frames (LDS)", lds_stage_floats(s.J), real);
        Buf<double> q5("q5 (LDS)", kStats * kMaxLimbs, real);
        for (int t0 = 0; t0 < s.T; t0 += TF) {
            const int n = TF < s.T - t0 ? TF : s.T - t0;
            const int64_t src = pred_frame(w, s.T, s.J, t0), block0 = pred_frame(w, s.T, s.J, 0),
                          block1 = block0 + (int64_t)s.T * J3;
            const int N = n * J3;
            int head, quads;
            stage_split(pred.addr + 4 * (uint64_t)src, N, head, quads);
            if (head < 0 || quads < 0 || head + 4 * quads > N) die("stage split", head + 4 * quads, N);
            if (src < block0 || src + N > block1) die("tile outside the sample's block", src, block1);
            for (int tid = 0; tid < kThreads; ++tid) {
                for (int e = tid; e < head; e += kThreads) fr.st(e, pred.ld(src + e));
                for (int q = tid; q < quads; q += kThreads) {
                    const float v = pred.ld(src + head + 4 * q, 4);
                    for (int k = 0; k < 4; ++k) fr.st(head + 4 * q + k, v);
                }
                for (int e = head + 4 * quads + tid; e < N; e += kThreads) fr.st(e, pred.ld(src + e));
            }
            for (int tid = 0; tid < kThreads; ++tid)
                for (int i = tid; i < n * s.L; i += kThreads) {
                    const int f = i / s.L, l = i - f * s.L;
                    joint(fr, f * J3, la[l]);
                    joint(fr, f * J3, lb[l]);
                    ll.st(i, 1.0);
                    if (with_target) {
                        joint(target, target_frame(b, s.T, s.J, t0 + f), la[l]);
                        joint(target, target_frame(b, s.T, s.J, t0 + f), lb[l]);
                        tl.st(i, 1.0);
                    }
                }
            for (int tid = 0; tid < s.L; ++tid)
                for (int f = 0; f < n; ++f) {
                    ll.ld(f * s.L + tid);
                    if (with_target) tl.ld(f * s.L + tid);
                    if (t0 + f > 0) {
                        steps.st(step_index(w, s.T, t0 + f, s.L, tid), 1.f);
                        if (with_target) diff.st(step_index(w, s.T, t0 + f, s.L, tid), 1.f);
                    }
                }
        }
        for (int tid = 0; tid < s.L; ++tid)
            for (int q = 0; q < kStats; ++q) {
                limb_out.st(limb_index(q, BS, w, s.L, tid), 1.f);
                q5.st(q * kMaxLimbs + tid, 1.0);
            }
        for (int tid = 0; tid < kSampleRows; ++tid) {
            const int op = sample_row_op(tid), stat = sample_row_stat(tid);
            if (op < 0 || op > 2 || stat < 0 || stat >= kStats) die("sample row tables", tid, kSampleRows);
            for (int l = 0; l < s.L; ++l) q5.ld(stat * kMaxLimbs + l);
            sample_out.st(sample_index(tid, BS, w), 1.f);
            scratch.st(sample_index(tid, BS, w), 1.0);
        }
    }
    // ---- k_limb_reduce: grid B, 64 threads ----
    for (int64_t b = 0; b < s.B; ++b)
        for (int r = 0; r < kSeqRows; ++r) {
            const int src = seq_row_source(r), op = seq_row_op(r);
            if (src < 0 || src >= kSampleRows || op < 0 || op > 2) die("sequence row tables", r, kSeqRows);
            for (int sm = 0; sm < s.S; ++sm) scratch.ld(sample_index(src, BS, b * s.S + sm));
            seq_out.st(seq_index(r, s.B, b), 1.f);
        }
}

struct FrameShape {
    int64_t R;
    int S, T, J, frame0, nframes;
};

// one row's span by its kCells lanes: every float of [0, N) copied exactly once, quads aligned and inside
void emulate_span(Buf<float>& src, int64_t off, int N, Buf<float>& dst, int row, std::vector<int>& seen) {
    int head, quads;
    stage_split(src.addr + 4 * (uint64_t)off, N, head, quads);
    if (head < 0 || quads < 0 || head + 4 * quads > N) die("span split", head + 4 * quads, N);
    if (quads > kCells) die("more quads than lanes", quads, kCells);
    seen.assign((size_t)N, 0);
    for (int k = 0; k < kCells; ++k) {
        int quad, scalar;
        span_lane(k, N, head, quads, quad, scalar);
        if (quad >= 0) {
            if (quad >= quads) die("quad past the split", quad, quads);
            const float v = src.ld(off + head + 4 * quad, 4);
            for (int i = 0; i < 4; ++i) {
                dst.st(lds_span(row, head + 4 * quad + i), v);
                ++seen[(size_t)(head + 4 * quad + i)];
            }
        }
        if (scalar >= 0) {
            if (scalar >= N) die("single float past the span", scalar, N);
            dst.st(lds_span(row, scalar), src.ld(off + scalar));
            ++seen[(size_t)scalar];
        }
    }
    for (int e = 0; e < N; ++e)
        if (seen[(size_t)e] != 1) die("span float not copied exactly once", e, seen[(size_t)e]);
}

void emulate_frame(const FrameShape& s, bool real, int phase, int bad_every) {
    const int J3 = 3 * s.J;
    Buf<float> pred("pred", s.R * s.S * s.T * J3, real, 0x10000 + 4 * (uint64_t)phase);
    Buf<float> target("target", s.R * s.T * J3, real, 0x20000 + 4 * (uint64_t)((phase + 1) & 3));
    const int64_t cells = cell_count(s.nframes, s.J);
    Buf<double> sum("sum", cells, real);
    Buf<double> count("count", 1, real);
    std::vector<int64_t> idx((size_t)s.R);
    for (int64_t r = 0; r < s.R; ++r)  // every sample, and now and then an index that is none
        idx[(size_t)r] = bad_every && r % bad_every == bad_every - 1 ? (r % 2 ? -1 - r : s.S + r) : r % s.S;
    std::vector<int> seen;
    const int64_t blocks = (cells + kCells - 1) / kCells;
    for (int64_t blk = 0; blk < blocks; ++blk) {
        const int64_t c0 = blk * kCells;
        const int nc = cells_of_block(cells, blk), N = 3 * nc;
        if (nc < 1 || nc > kCells) die("cells of a block", nc, kCells);
        Buf<float> ps("ps (LDS)", kRows * kSpanFloats, real), ts("ts (LDS)", kRows * kSpanFloats, real);
        Buf<double> en("en (LDS)", kRows * kCells, real);
        for (int tid = 0; tid < nc; ++tid) sum.ld(c0 + tid);
        for (int64_t r0 = 0; r0 < s.R; r0 += kRows) {
            const int nr = (int)(s.R - r0 < kRows ? s.R - r0 : kRows);
            for (int pr = 0; pr < nr; ++pr) {
                const int64_t r = r0 + pr;
                const int smp = sample_or_none(idx[(size_t)r], s.S);
                if (smp >= s.S) die("sample index", smp, s.S);
                if (smp >= 0) {
                    const int64_t off = pred_span(r, smp, s.S, s.T, s.J, s.frame0, c0);
                    const int64_t lo = ((r * s.S + smp) * s.T + s.frame0) * J3, hi = lo + (int64_t)s.nframes * J3;
                    if (off < lo || off + N > hi) die("span outside the row's window", off, hi);
                    emulate_span(pred, off, N, ps, pr, seen);
                }
                emulate_span(target, target_span(r, s.T, s.J, s.frame0, c0), N, ts, pr, seen);
                for (int k = 0; k < nc; ++k) {
                    if (smp >= 0)
                        for (int i = 0; i < 3; ++i) {
                            ps.ld(lds_span(pr, 3 * k + i));
                            ts.ld(lds_span(pr, 3 * k + i));
                        }
                    en.st(lds_cell(pr, k), 1.0);
                }
            }
            for (int tid = 0; tid < nc; ++tid)
                for (int i = 0; i < nr; ++i) en.ld(lds_cell(i, tid));
        }
        for (int tid = 0; tid < nc; ++tid) sum.st(c0 + tid, 1.0);
        if (blk == 0) count.st(0, count.ld(0) + (double)s.R);
    }
}

void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "arithmetic check failed: %s\n", what);
        std::abort();
    }
}

// the combine step against a two-pass variance: near-rigid lengths (0.3 +- 1e-2), every tile size, T up to 130
void check_arithmetic() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(rng >> 11) / 9007199254740992.0;
    };
    for (int T : {1, 2, 3, 13, 14, 32, 33, 64, 100, 130})
        for (int tile : {1, 10, 13, 32}) {
            std::vector<double> x((size_t)T);
            for (double& v : x) v = 0.3 + 1e-2 * (next() - 0.5);
            double mean = 0.0;
            for (double v : x) mean += v;
            mean /= T;
            double m2 = 0.0;
            for (double v : x) m2 += (v - mean) * (v - mean);
            double cn = 0.0, cmean = 0.0, cm2 = 0.0;
            for (int t0 = 0; t0 < T; t0 += tile) {
                const int n = tile < T - t0 ? tile : T - t0;
                double sm = 0.0, tm2 = 0.0;
                for (int f = 0; f < n; ++f) sm += x[(size_t)(t0 + f)];
                const double tmean = sm / n;
                for (int f = 0; f < n; ++f) tm2 += (x[(size_t)(t0 + f)] - tmean) * (x[(size_t)(t0 + f)] - tmean);
                var_combine(cn, cmean, cm2, (double)n, tmean, tm2);
            }
            check(cn == (double)T, "combined count");
            check(std::fabs(cmean - mean) <= 1e-14, "combined mean");  // T eps |x| = 130 x 1.1e-16 x 0.3 = 4e-15
            check(std::fabs(cm2 - m2) <= 1e-12 * m2, "combined sum of squares within 1e-12 of two passes");
            if (T == 1) check(cm2 == 0.0 && std::isnan(cm2 / (double)(T - 1)), "one frame: 0 / 0");
        }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    check(max_keep_nan(1.0, 2.0) == 2.0 && max_keep_nan(2.0, 1.0) == 2.0 && min_keep_nan(1.0, 2.0) == 1.0 &&
              min_keep_nan(2.0, 1.0) == 1.0, "maximum / minimum of numbers");
    check(std::isnan(max_keep_nan(nan, 1.0)) && std::isnan(max_keep_nan(1.0, nan)) && std::isnan(min_keep_nan(nan, 1.0)) &&
              std::isnan(min_keep_nan(1.0, nan)), "maximum / minimum keep NaN");
    const double inf = std::numeric_limits<double>::infinity();
    check(max_keep_nan(-inf, inf) == inf && min_keep_nan(inf, -inf) == -inf, "maximum / minimum of infinities");
    check(sample_or_none(0, 7) == 0 && sample_or_none(6, 7) == 6 && sample_or_none(7, 7) == -1 && sample_or_none(-1, 7) == -1 &&
              sample_or_none(INT64_MAX, 64) == -1 && sample_or_none(INT64_MIN, 64) == -1 &&
              sample_or_none((int64_t)1 << 32, 64) == -1, "sample index clamp");
}

}  // namespace

int main() {
    check_arithmetic();
    // the fixture's shapes and the tests' ragged ones on real buffers, pred at each of the four 16-byte phases
    const LimbShape limb_small[] = {
        {2, 7, 20, 16, 15}, {2, 5, 33, 21, 20}, {1, 3, 4, 51, 50}, {1, 2, 5, 17, 16}, {2, 7, 2, 16, 15}, {2, 7, 1, 16, 15},
        {1, 2, 67, 64, 64}, {1, 64, 14, 51, 50}, {1, 1, 65, 1, 1},  {1, 1, 33, 16, 1},
    };
    for (const LimbShape& s : limb_small)
        for (int phase = 0; phase < 4; ++phase) {
            emulate_limb(s, true, phase, true);
            emulate_limb(s, true, phase, false);
        }
    const FrameShape frame_small[] = {
        {1, 1, 1, 16, 0, 1},  {5, 7, 2, 21, 0, 2},   {33, 7, 31, 51, 0, 31}, {37, 3, 61, 16, 0, 61}, {37, 3, 61, 16, 60, 1},
        {5, 1, 31, 51, 30, 1}, {17, 64, 3, 64, 1, 2}, {16, 2, 5, 1, 0, 5},    {3, 2, 7, 17, 2, 4},
    };
    for (const FrameShape& s : frame_small)
        for (int phase = 0; phase < 4; ++phase) {
            emulate_frame(s, true, phase, 0);
            emulate_frame(s, true, phase, 3);
        }
    // the validation's shapes, indices checked arithmetically
    emulate_limb({8, 50, 100, 16, 15}, false, 0, true);
    emulate_limb({256, 50, 120, 21, 20}, false, 3, false);
    emulate_frame({256, 50, 100, 16, 0, 100}, false, 1, 0);
    emulate_frame({256, 50, 120, 21, 119, 1}, false, 2, 5);
    std::printf("validation emulation ok: %lld accesses in bounds\n", g_accesses);
    return 0;
}
