// Host emulation of sd_rank.hip with the functions of skeletondiffusion_amd/csrc/sd_rank_addr.h, the same ones
// the kernels call.
//   Phase 1 (k_rank_dist): every workgroup x thread x load / LDS slot / store for samples + 1 in {2, 63, 64,
//   65, 256} and features in {1, 9, 32, 33}.  Every buffer is a heap allocation of its exact size (build with
//   -fsanitize=address,undefined: an access outside one aborts); an LDS slot is written once per chunk and
//   read only after it was written; every entry of the distance matrix is written exactly once; the matrix
//   equals, bit for bit, the chunked float chain of sd_cdist formed directly from the two rows, is symmetric
//   with a zero diagonal, and lies within the bound of a float sum of `features` squares of a double
//   restatement.
//   Phase 2 (k_rank_select): the workgroup's 256 threads in lockstep, the xor butterfly and the wave order of
//   the kernel, on matrices with ties (values on a coarse grid, duplicated points) and NaN rows, with and
//   without from_closest, against a restatement with double keys that follows the specification literally.
// Built and run by tests/test_rank_host.py; no GPU, nothing preloaded.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_rank_addr.h"

using namespace sd::rank;

namespace {

[[noreturn]] void die(const char* what, int64_t a, int64_t b) {
    std::fprintf(stderr, "rank emulation: %s (%" PRId64 ", %" PRId64 ")\n", what, a, b);
    std::abort();
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
float rnd_unit() { return (float)(rnd() & 0xFFFFFF) / (float)0x1000000 * 2.f - 1.f; }

struct Quad {
    float c[4];
};

// sd_cdist's value function on two rows
float chain(const float* a, const float* b, int64_t features) {
    float acc = 0.f;
    for (int64_t k0 = 0; k0 < features; k0 += kKC) {
        float t = 0.f;
        for (int64_t k = k0; k < features && k < k0 + kKC; ++k) {
            const float d = a[k] - b[k];
            t = std::fmaf(d, d, t);
        }
        acc = acc + t;
    }
    return std::sqrt(acc);
}

int64_t walk_phase1(int64_t nseq, int points, int64_t features) {
    const int samples = points - 1;
    std::vector<float> pred((size_t)(nseq * samples * features)), target((size_t)(nseq * features));
    for (float& v : pred) v = rnd_unit();
    for (float& v : target) v = rnd_unit();
    std::vector<float> dist((size_t)(nseq * points * points), -1.f);
    std::vector<uint8_t> written(dist.size(), 0);
    int64_t accesses = 0;

    auto point = [&](int64_t b, int pt) -> const float* {
        const int64_t off = point_offset(b, pt, samples, features);
        const std::vector<float>& src = pt == 0 ? target : pred;
        if (off < 0 || off + features > (int64_t)src.size()) die("row outside its tensor", off, (int64_t)src.size());
        return src.data() + off;
    };
    auto load_quad = [&](int64_t b, int pt, int64_t k) {  // the kernel's load_quad, element by element
        Quad q = {{0.f, 0.f, 0.f, 0.f}};
        if (pt < points && k < features) {
            const float* p = point(b, pt);
            for (int c = 0; c < 4; ++c)
                if (k + c < features) {
                    q.c[c] = p[k + c];  // read through the raw pointer: the sanitizer sees it
                    ++accesses;
                }
        }
        return q;
    };
    auto store = [&](int64_t off, float v) {
        if (off < 0 || off >= (int64_t)dist.size()) die("dist store outside the matrix", off, (int64_t)dist.size());
        if (written[(size_t)off]++) die("dist entry written twice", off, 0);
        dist.data()[off] = v;
        ++accesses;
    };

    const int ntiles = tiles(points), npairs = tile_pairs(points);
    std::vector<uint8_t> seen((size_t)(ntiles * ntiles), 0);
    const int64_t nchunks = (features + kKC - 1) / kKC;
    for (int64_t wg = 0; wg < nseq * npairs; ++wg) {
        const int64_t b = wg / npairs;
        int ti, tj;
        pair_tiles((int)(wg - b * npairs), ntiles, &ti, &tj);
        if (ti < 0 || tj < ti || tj >= ntiles) die("tile pair outside the upper triangle", ti, tj);
        if (b == 0 && seen[(size_t)(ti * ntiles + tj)]++) die("tile pair visited twice", ti, tj);
        const int i0 = ti * kTile, j0 = tj * kTile;
        std::vector<float> acc((size_t)(kDistThreads * kOut * kOut), 0.f);
        for (int64_t c = 0; c < nchunks; ++c) {
            std::vector<Quad> As((size_t)(kKQ * kLd)), Bs((size_t)(kKQ * kLd));
            std::vector<uint8_t> wa(As.size(), 0), wb(Bs.size(), 0);
            for (int tid = 0; tid < kDistThreads; ++tid)
                for (int q = 0; q < kQ; ++q) {
                    const int r = load_row(tid, q), kq = load_kq(tid);
                    if (r < 0 || r >= kTile || kq < 0 || kq >= kKQ) die("loader role outside the tile", r, kq);
                    const int sa = a_slot(kq, r), sb = b_slot(kq, r);
                    if (sa < 0 || sa >= (int)As.size() || wa[(size_t)sa]++) die("A slot outside LDS or written twice", sa, tid);
                    if (sb < 0 || sb >= (int)Bs.size() || wb[(size_t)sb]++) die("B slot outside LDS or written twice", sb, tid);
                    As[(size_t)sa] = load_quad(b, i0 + r, c * kKC + 4 * kq);
                    Bs[(size_t)sb] = load_quad(b, j0 + r, c * kKC + 4 * kq);
                }
            const int nkq = chunk_quads(features, c);
            if (nkq < 1 || nkq > kKQ) die("chunk without a k quad", nkq, c);
            for (int tid = 0; tid < kDistThreads; ++tid) {
                float t[kOut][kOut] = {};
                for (int kq = 0; kq < nkq; ++kq)
                    for (int kk = 0; kk < 4; ++kk)
                        for (int i = 0; i < kOut; ++i)
                            for (int j = 0; j < kOut; ++j) {
                                const int sa = a_slot(kq, out_row(tid, i)), sb = b_slot(kq, out_col(tid, j));
                                if (sa < 0 || sa >= (int)As.size() || !wa[(size_t)sa]) die("A slot read before written", sa, tid);
                                if (sb < 0 || sb >= (int)Bs.size() || !wb[(size_t)sb]) die("B slot read before written", sb, tid);
                                const float d = As[(size_t)sa].c[kk] - Bs[(size_t)sb].c[kk];
                                t[i][j] = std::fmaf(d, d, t[i][j]);
                            }
                for (int i = 0; i < kOut; ++i)
                    for (int j = 0; j < kOut; ++j) {
                        float& a = acc[(size_t)((tid * kOut + i) * kOut + j)];
                        a = a + t[i][j];
                    }
            }
        }
        for (int tid = 0; tid < kDistThreads; ++tid)
            for (int i = 0; i < kOut; ++i)
                for (int j = 0; j < kOut; ++j) {
                    const int gi = i0 + out_row(tid, i), gj = j0 + out_col(tid, j);
                    if (!owns(ti, tj, gi, gj, points)) continue;
                    const float v = std::sqrt(acc[(size_t)((tid * kOut + i) * kOut + j)]);
                    store(dist_offset(b, points, gi, gj), v);
                    if (gi != gj) store(dist_offset(b, points, gj, gi), v);
                }
    }
    for (int ti = 0; ti < ntiles; ++ti)
        for (int tj = ti; tj < ntiles; ++tj)
            if (!seen[(size_t)(ti * ntiles + tj)]) die("tile pair never visited", ti, tj);
    for (size_t e = 0; e < written.size(); ++e)
        if (written[e] != 1) die("dist entry not written", (int64_t)e, written[e]);
    for (int64_t b = 0; b < nseq; ++b)
        for (int i = 0; i < points; ++i)
            for (int j = 0; j < points; ++j) {
                const float got = dist[(size_t)dist_offset(b, points, i, j)];
                const float want = chain(point(b, i), point(b, j), features);
                if (std::memcmp(&got, &want, 4) != 0) die("entry differs from the chunked chain", i, j);
                const float mirror = dist[(size_t)dist_offset(b, points, j, i)];
                if (std::memcmp(&got, &mirror, 4) != 0) die("matrix not symmetric", i, j);
                if (i == j && got != 0.f) die("diagonal not zero", i, j);
                double s = 0.0;
                for (int64_t k = 0; k < features; ++k) {
                    const double d = (double)point(b, i)[k] - (double)point(b, j)[k];
                    s += d * d;
                }
                const double ref = std::sqrt(s), tol = (double)(features + 4) * std::ldexp(1.0, -24) * ref;
                if (std::fabs((double)got - ref) > tol) die("entry outside the float bound of the double value", i, j);
            }
    return accesses;
}

// ---- phase 2 ----------------------------------------------------------------------------------------------
// the kernel's group_best on 256 lockstep threads
template <bool MAX>
int group_best(std::vector<float> v, std::vector<int> i, float* best) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const std::vector<float> pv = v;
        const std::vector<int> pi = i;
        for (int t = 0; t < kThreads; ++t) {
            const int partner = (t & ~(kWave - 1)) | ((t & (kWave - 1)) ^ o);
            meet<MAX>(&v[(size_t)t], &i[(size_t)t], pv[(size_t)partner], pi[(size_t)partner]);
        }
    }
    float wv[kThreads / kWave];
    int wi[kThreads / kWave];
    for (int w = 0; w < kThreads / kWave; ++w) {
        for (int l = 1; l < kWave; ++l)  // every lane of a wave holds the wave's winner
            if (i[(size_t)(w * kWave + l)] != i[(size_t)(w * kWave)]) die("lanes of a wave disagree", w, l);
        wv[w] = v[(size_t)(w * kWave)];
        wi[w] = i[(size_t)(w * kWave)];
    }
    float bv;
    int bi;
    block_best<MAX>(wv, wi, kThreads / kWave, &bv, &bi);
    *best = bv;
    return bi;
}

struct Picks {
    std::vector<int64_t> idx;
    std::vector<float> score;
    int64_t closest = -1;
    std::vector<float> dist_out;
};

Picks emulate_select(const std::vector<float>& D, int points, int n_choose, bool from_closest) {
    Picks out;
    std::vector<float> m((size_t)kThreads, 0.f);
    std::vector<bool> live((size_t)kThreads);
    auto at = [&](int64_t r, int c) -> float {
        const int64_t off = r * points + c;
        if (off < 0 || off >= (int64_t)D.size()) die("select reads outside the matrix", off, (int64_t)D.size());
        return D.data()[off];
    };
    for (int t = 0; t < kThreads; ++t) live[(size_t)t] = t >= 1 && t < points;
    int anchor = 0;
    float best;
    std::vector<float> v((size_t)kThreads);
    std::vector<int> ix((size_t)kThreads);
    if (from_closest) {
        for (int t = 0; t < kThreads; ++t) {
            v[(size_t)t] = live[(size_t)t] ? at(0, t) : 0.f;
            ix[(size_t)t] = live[(size_t)t] ? t : -1;
        }
        anchor = group_best<false>(v, ix, &best);
        out.closest = anchor - 1;
    }
    for (int t = 0; t < kThreads; ++t) m[(size_t)t] = live[(size_t)t] ? at(anchor, t) : 0.f;
    for (int k = 0; k < n_choose; ++k) {
        for (int t = 0; t < kThreads; ++t) {
            v[(size_t)t] = m[(size_t)t];
            ix[(size_t)t] = live[(size_t)t] ? t : -1;
        }
        const int c = group_best<true>(v, ix, &best);
        if (c < 1 || c >= points) die("pick outside the samples", c, points);
        out.idx.push_back(c - 1);
        out.score.push_back(best);
        live[(size_t)c] = false;
        for (int t = 0; t < kThreads; ++t)
            if (live[(size_t)t]) m[(size_t)t] = min_nan(m[(size_t)t], at(c, t));
    }
    out.dist_out.resize(D.size());
    for (int e = 0; e < points * points; ++e) {
        const int i = e / points, j = e - i * points;
        out.dist_out[(size_t)e] = at(anchored(i, anchor), anchored(j, anchor));
    }
    return out;
}

// The specification, literally, with double keys: NaN -> -infinity for the arg-max (below every number),
// +infinity for the arg-min of the closest sample (above every number); the first index of the extremum.
Picks restate_select(const std::vector<float>& D, int points, int n_choose, bool from_closest) {
    const double inf = std::numeric_limits<double>::infinity();
    Picks out;
    auto d = [&](int i, int j) { return D[(size_t)i * (size_t)points + (size_t)j]; };
    int anchor = 0;
    if (from_closest) {
        double bestk = 0;
        for (int s = 1; s < points; ++s) {
            const double key = std::isnan(d(0, s)) ? inf : (double)d(0, s);
            if (anchor == 0 || key < bestk) {
                anchor = s;
                bestk = key;
            }
        }
        out.closest = anchor - 1;
    }
    std::vector<float> m((size_t)points);
    std::vector<bool> in_c((size_t)points, false);
    in_c[0] = true;
    for (int i = 1; i < points; ++i) m[(size_t)i] = d(i, anchor);
    for (int k = 0; k < n_choose; ++k) {
        int c = -1;
        double bestk = 0;
        for (int i = 1; i < points; ++i) {
            if (in_c[(size_t)i]) continue;
            const double key = std::isnan(m[(size_t)i]) ? -inf : (double)m[(size_t)i];
            if (c < 0 || key > bestk) {
                c = i;
                bestk = key;
            }
        }
        out.idx.push_back(c - 1);
        out.score.push_back(m[(size_t)c]);
        in_c[(size_t)c] = true;
        for (int i = 1; i < points; ++i) {
            const float a = m[(size_t)i], b2 = d(i, c);
            m[(size_t)i] = std::isnan(a) || std::isnan(b2) ? std::numeric_limits<float>::quiet_NaN() : std::fmin(a, b2);
        }
    }
    return out;
}

bool same_float(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

int walk_phase2(int points, int variant) {
    // points on a line at grid positions: many equal distances; variant 1 duplicates points, 2 adds NaN
    // points, 3 makes all points equal
    std::vector<float> pos((size_t)points);
    for (int i = 0; i < points; ++i) pos[(size_t)i] = variant == 3 ? 1.f : (float)(rnd() % 17) * 0.25f;
    if (variant == 1)
        for (int i = 2; i < points; i += 3) pos[(size_t)i] = pos[(size_t)(i - 1)];
    if (variant == 2)
        for (int i = 1; i < points; i += 5) pos[(size_t)i] = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> D((size_t)points * (size_t)points);
    for (int i = 0; i < points; ++i)
        for (int j = 0; j < points; ++j) D[(size_t)i * (size_t)points + (size_t)j] = std::fabs(pos[(size_t)i] - pos[(size_t)j]);
    int cases = 0;
    const int samples = points - 1;
    for (int n : {1, samples / 2, samples}) {
        if (n < 1) continue;
        for (int fc = 0; fc < 2; ++fc) {
            const Picks a = emulate_select(D, points, n, fc != 0), b = restate_select(D, points, n, fc != 0);
            if (a.closest != b.closest) die("closest differs from the restatement", a.closest, b.closest);
            for (int k = 0; k < n; ++k) {
                if (a.idx[(size_t)k] != b.idx[(size_t)k]) die("pick differs from the restatement", k, a.idx[(size_t)k]);
                if (!same_float(a.score[(size_t)k], b.score[(size_t)k])) die("score differs from the restatement", k, points);
            }
            std::vector<uint8_t> used((size_t)samples, 0);
            for (int64_t s : a.idx)
                if (s < 0 || s >= samples || used[(size_t)s]++) die("a sample picked twice or out of range", s, samples);
            if (variant == 3)
                for (int k = 0; k < n; ++k)
                    if (a.idx[(size_t)k] != k) die("all-equal samples not picked in index order", k, a.idx[(size_t)k]);
            if (variant == 2 && n == samples) {  // the NaN samples come after every number
                bool nan_seen = false;
                for (int64_t s : a.idx) {
                    const bool is = std::isnan(pos[(size_t)(s + 1)]);
                    if (nan_seen && !is && !std::isnan(pos[0]) && !(fc && std::isnan(pos[(size_t)(a.closest + 1)])))
                        die("a number picked after a NaN sample", s, points);
                    nan_seen = nan_seen || is;
                }
            }
            const int anchor = fc ? (int)a.closest + 1 : 0;
            for (int i = 0; i < points; ++i)
                for (int j = 0; j < points; ++j)
                    if (!same_float(a.dist_out[(size_t)i * (size_t)points + (size_t)j],
                                    std::fabs(pos[(size_t)(i ? i : anchor)] - pos[(size_t)(j ? j : anchor)])))
                        die("anchored matrix differs", i, j);
            ++cases;
        }
    }
    return cases;
}

}  // namespace

int main() {
    static_assert(kMaxPoints <= kThreads, "one selection thread per point");
    static_assert(kTile * kKQ == kQ * kDistThreads && kOut * 8 == kTile, "phase 1 roles cover the tile");
    int cases = 0;
    int64_t accesses = 0;
    for (int points : {2, 63, 64, 65, 256})
        for (int64_t features : {1, 9, 32, 33}) {
            accesses += walk_phase1(points == 256 ? 1 : 2, points, features);
            ++cases;
        }
    int select_cases = 0;
    for (int points : {2, 3, 63, 64, 65, 130, 256})
        for (int variant = 0; variant < 4; ++variant) select_cases += walk_phase2(points, variant);
    std::printf("rank emulation ok (%d matrix cases, %" PRId64 " accesses, %d selection cases)\n", cases, accesses, select_cases);
    return 0;
}
