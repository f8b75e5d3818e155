// Host emulation of sd_q_sample.hip (k_q_sample_groups): every workgroup x thread x load / store of the
// kernel's two passes, with the offsets, LDS indices, loop bounds, the row -> (sequence, copy) -> Philox-row
// map and the sums of skeletondiffusion_amd/csrc/sd_q_sample_addr.h, the same functions the kernel calls.
// Every buffer is a heap allocation of its exact size (build with -fsanitize=address,undefined: an access
// outside one aborts), every 16-byte access must be 16-byte aligned, every element of x_t and noise_out must
// be written exactly once, every (row, quad) of a `sel` launch must use the Philox counter the full launch
// uses for that row, its rows must equal the full launch's bit for bit, and x_t must lie within the bound of
// an f32 sum of J + 1 products of a restatement in double.  t and sel hold out-of-range values: they are
// clamped, not read out of bounds.  Built and run by tests/test_selected_step.py; no GPU, nothing preloaded.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_q_sample_addr.h"

using namespace sd::qsample;

namespace {

long long g_accesses = 0;

[[noreturn]] void die(const char* what, int64_t idx, int64_t size) {
    std::fprintf(stderr, "q_sample emulation: %s (index %" PRId64 ", size %" PRId64 ")\n", what, idx, size);
    std::abort();
}

template <class E>
struct Buf {
    const char* name;
    std::vector<E> v;
    std::vector<uint8_t> count;  // outputs: how often each element was written
    Buf(const char* n, int64_t size, bool counted = false) : name(n), v((size_t)size) {
        if (counted) count.assign((size_t)size, 0);
    }
    int64_t size() const { return (int64_t)v.size(); }
    void span(int64_t i, int width) const {
        if (i < 0 || i + width > size()) die(name, i, size());
        if (width > 1 && (i * sizeof(E)) % (sizeof(E) * width)) die("misaligned vector access", i, size());
    }
    const E* ld(int64_t i, int width = 1) const {
        span(i, width);
        g_accesses += width;
        return v.data() + i;  // read through the raw pointer: the sanitizer sees it
    }
    void st(int64_t i, const E* src, int width) {
        span(i, width);
        g_accesses += width;
        for (int c = 0; c < width; ++c) {
            v.data()[i + c] = src[c];
            if (!count.empty() && ++count[(size_t)(i + c)] != 1) die("written twice", i + c, size());
        }
    }
    void all_written() const {
        for (int64_t i = 0; i < size(); ++i)
            if (count[(size_t)i] != 1) die("not written", i, size());
    }
};

// a stand-in for box_muller(philox_at(seed, row, step, quad)): any function of (row, quad, lane)
float fake_normal(uint64_t row, uint32_t quad, int c) {
    uint64_t h = (row + 1) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)quad * 4 + (uint64_t)c + 7) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return (float)((double)(h & 0xFFFFFF) / (double)0x1000000 * 6.0 - 3.0);
}

struct Shape {
    int64_t nseq;
    int k, J, D;
};

struct Inputs {
    Shape s;
    int T;
    int64_t row0;
    Buf<float> x0, sqrt_ac, M, sqrt_1mac;
    Buf<int64_t> t, sel;
    Inputs(Shape sh, int T_, int64_t row0_)
        : s(sh), T(T_), row0(row0_), x0("x0", sh.nseq * sh.J * sh.D), sqrt_ac("sqrt_alphas_cumprod", T_),
          M("M", (int64_t)T_ * sh.J * sh.J), sqrt_1mac("sqrt_one_minus_alphas_cumprod", T_), t("t", sh.nseq),
          sel("sel", sh.nseq) {
        for (int64_t i = 0; i < x0.size(); ++i) x0.v[(size_t)i] = fake_normal(991, (uint32_t)(i >> 2), (int)(i & 3)) * 0.4f;
        for (int i = 0; i < T; ++i) {
            sqrt_ac.v[(size_t)i] = 0.95f - 0.9f * (float)i / (float)T;
            sqrt_1mac.v[(size_t)i] = std::sqrt(1.f - sqrt_ac.v[(size_t)i] * sqrt_ac.v[(size_t)i]);
        }
        for (int64_t i = 0; i < M.size(); ++i) M.v[(size_t)i] = fake_normal(17, (uint32_t)(i >> 2), (int)(i & 3)) * 0.3f;
        // timesteps 0 and T - 1 and values outside [0, T); selections outside [0, k)
        const int64_t ts[] = {0, T - 1, T / 2, -3, T + 5};
        const int64_t ss[] = {0, sh.k - 1, sh.k / 2, -1, sh.k + 2};
        for (int64_t i = 0; i < sh.nseq; ++i) {
            t.v[(size_t)i] = ts[i % 5];
            sel.v[(size_t)i] = ss[(i + 1) % 5];
        }
    }
};

struct Launch {
    Buf<float> x_t, noise_out;
    std::vector<uint64_t> philox_row;  // per output row
    Launch(int64_t rows, int JD) : x_t("x_t", rows * JD, true), noise_out("noise_out", rows * JD, true), philox_row((size_t)rows) {}
};

// the kernel, one workgroup after another, every thread of it in turn per pass
void run(const Inputs& in, bool mixing, bool has_sel, const Buf<float>* noise_in, Launch& out) {
    const int J = in.s.J, D = in.s.D, k = in.s.k, Q = quads(J, D);
    if (Q * 4 != J * D) die("quads do not cover the row", Q, J * D);
    const int64_t rows = out_rows(in.s.nseq, k, has_sel);
    Buf<float> lds("LDS", (int64_t)lds_floats(J, D, mixing));
    if (lds.size() * 4 > 65536) die("LDS above 64 KiB", lds.size() * 4, 65536);
    for (int64_t o = 0; o < rows; ++o) {
        const RowMap rm = row_map(o, k, has_sel, has_sel ? *in.sel.ld(o) : 0, in.row0);
        if (rm.seq < 0 || rm.seq >= in.s.nseq || rm.copy < 0 || rm.copy >= k) die("row map", rm.seq, in.s.nseq);
        if (rm.noise_row != rm.seq * k + rm.copy || rm.philox_row != (uint64_t)(in.row0 + rm.noise_row))
            die("Philox row", rm.noise_row, rows);
        out.philox_row[(size_t)o] = rm.philox_row;
        const int t = clamp_t(*in.t.ld(rm.seq), in.T);
        const float ca = *in.sqrt_ac.ld(t);
        const float cb = mixing ? 0.f : *in.sqrt_1mac.ld(t);
        for (int tid = 0; tid < kThreads; ++tid)
            for (int q = tid; q < Q; q += kThreads) {
                const int e = quad_elem(q);
                float v[4];
                if (noise_in) std::memcpy(v, noise_in->ld(row_elem(rm.noise_row, J, D, e), 4), sizeof v);
                else
                    for (int c = 0; c < 4; ++c) v[c] = fake_normal(rm.philox_row, (uint32_t)q, c);
                out.noise_out.st(row_elem(o, J, D, e), v, 4);
                if (mixing) {
                    lds.st(e, v, 4);
                } else {
                    float r[4];
                    iso_quad(ca, in.x0.ld(row_elem(rm.seq, J, D, e), 4), cb, v, r);
                    out.x_t.st(row_elem(o, J, D, e), r, 4);
                }
            }
        if (!mixing) continue;
        for (int tid = 0; tid < kThreads; ++tid)
            for (int q = tid; q < Q; q += kThreads) {
                const int i = item_joint(q, D), d0 = item_d0(q, D), e = i * D + d0;
                if (i < 0 || i >= J || d0 < 0 || d0 + 4 > D) die("mixing item", q, Q);
                in.M.ld(m_row(t, J, i), 1);
                in.M.ld(m_row(t, J, i) + J - 1, 1);
                for (int j = 0; j < J; ++j) lds.ld((int64_t)j * D + d0, 4);
                float r[4];
                mix_quad(ca, in.x0.ld(row_elem(rm.seq, J, D, e), 4), in.M.v.data() + m_row(t, J, i), lds.v.data(), J, D, d0, r);
                out.x_t.st(row_elem(o, J, D, e), r, 4);
            }
    }
    out.x_t.all_written();
    out.noise_out.all_written();
}

// x_t against the expression in double on the launch's own noise_out
void check_values(const Inputs& in, bool mixing, bool has_sel, const Launch& L) {
    const int J = in.s.J, D = in.s.D, k = in.s.k;
    const int64_t rows = out_rows(in.s.nseq, k, has_sel);
    const double u = std::ldexp(1.0, -24);
    for (int64_t o = 0; o < rows; ++o) {
        const int64_t s = has_sel ? o : o / k;
        int64_t tt = in.t.v[(size_t)s];
        tt = tt < 0 ? 0 : (tt > in.T - 1 ? in.T - 1 : tt);
        const double a = in.sqrt_ac.v[(size_t)tt], b = in.sqrt_1mac.v[(size_t)tt];
        for (int i = 0; i < J; ++i)
            for (int d = 0; d < D; ++d) {
                const double x0 = in.x0.v[(size_t)((s * J + i) * D + d)];
                double ref = a * x0, mag = std::fabs(a * x0);
                if (mixing) {
                    for (int j = 0; j < J; ++j) {
                        const double p = (double)in.M.v[(size_t)((tt * J + i) * J + j)] * (double)L.noise_out.v[(size_t)((o * J + j) * D + d)];
                        ref += p;
                        mag += std::fabs(p);
                    }
                } else {
                    const double p = b * (double)L.noise_out.v[(size_t)((o * J + i) * D + d)];
                    ref += p;
                    mag += std::fabs(p);
                }
                const double got = L.x_t.v[(size_t)((o * J + i) * D + d)];
                if (std::fabs(got - ref) > (J + 2) * u * mag) die("x_t differs from the restatement in double", (o * J + i) * D + d, rows);
            }
    }
}

}  // namespace

int main() {
    const Shape shapes[] = {{1, 1, 1, 4}, {3, 4, 16, 96}, {2, 50, 17, 96}, {5, 7, 21, 96}, {1, 3, 51, 96}, {2, 2, 64, 256}};
    int variants = 0;
    for (const Shape& sh : shapes)
        for (int mixing = 0; mixing < 2; ++mixing) {
            const Inputs in(sh, 10, 1000003);
            const int JD = sh.J * sh.D;
            Launch full(sh.nseq * sh.k, JD), picked(sh.nseq, JD), fed(sh.nseq * sh.k, JD), fed_picked(sh.nseq, JD);
            run(in, mixing != 0, false, nullptr, full);
            run(in, mixing != 0, true, nullptr, picked);
            run(in, mixing != 0, false, &full.noise_out, fed);        // noise_in = the noise the full launch drew
            run(in, mixing != 0, true, &full.noise_out, fed_picked);
            check_values(in, mixing != 0, false, full);
            check_values(in, mixing != 0, true, picked);
            // the full launch keys row r with row0 + r; a sel launch uses the counters and returns the bits of its rows
            for (int64_t r = 0; r < sh.nseq * sh.k; ++r)
                if (full.philox_row[(size_t)r] != (uint64_t)(in.row0 + r)) die("full launch Philox row", r, sh.nseq * sh.k);
            for (int64_t s = 0; s < sh.nseq; ++s) {
                const int64_t r = s * sh.k + clamp_sel(in.sel.v[(size_t)s], sh.k);
                if (picked.philox_row[(size_t)s] != full.philox_row[(size_t)r]) die("sel launch Philox row", s, sh.nseq);
                if (std::memcmp(&picked.x_t.v[(size_t)(s * JD)], &full.x_t.v[(size_t)(r * JD)], sizeof(float) * JD) ||
                    std::memcmp(&picked.noise_out.v[(size_t)(s * JD)], &full.noise_out.v[(size_t)(r * JD)], sizeof(float) * JD))
                    die("sel launch differs from the full launch's row", s, sh.nseq);
                if (std::memcmp(&fed_picked.x_t.v[(size_t)(s * JD)], &full.x_t.v[(size_t)(r * JD)], sizeof(float) * JD))
                    die("sel launch on supplied noise differs from the full launch's row", s, sh.nseq);
            }
            if (std::memcmp(fed.x_t.v.data(), full.x_t.v.data(), sizeof(float) * full.x_t.v.size()))
                die("supplied noise gives other bits than the launch that drew it", 0, full.x_t.size());
            variants += 4;
        }
    std::printf("q_sample emulation ok (%d launches, %lld accesses)\n", variants, g_accesses);
    return 0;
}
