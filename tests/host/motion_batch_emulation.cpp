// Host emulation of the address arithmetic of sd_motion_batch.hip (k_motion_batch, k_motion_draws): every
// workgroup x thread x load / store of the two kernels, with the offsets, LDS indices and loop bounds of
// skeletondiffusion_amd/csrc/sd_motion_batch_addr.h, the same functions the kernels call.  Small shapes run on
// real heap buffers of the exact sizes (build with -fsanitize=address,undefined: an access outside one
// aborts); large shapes check every index against the buffer's size arithmetically.  16-byte accesses must be
// 16-byte aligned and stay inside the span they belong to; every element of obs, pred, segment_idx and the draw
// tensors must be written exactly once.  Built and run by tests/test_motion_batch_host.py; no GPU, nothing
// preloaded.
//
//   motion_batch_emulation            all built-in shapes
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_motion_batch_addr.h"

using namespace sd::motion;

namespace {

long long g_accesses = 0;

[[noreturn]] void die(const char* what, int64_t idx, int64_t size) {
    std::fprintf(stderr, "out of bounds: %s index %" PRId64 " size %" PRId64 "\n", what, idx, size);
    std::abort();
}

// a buffer of `size` elements of type E at a pretended byte address; `real` holds it on the heap or is empty;
// `count` (outputs only) holds how often each element was written
template <class E>
struct Buf {
    const char* name;
    int64_t size;
    uint64_t addr;  // pretended device address of element 0
    std::vector<E> real;
    std::vector<uint8_t> count;
    Buf(const char* n, int64_t s, bool make_real, uint64_t a = 0x10000, bool counted = false) : name(n), size(s), addr(a) {
        if (make_real) real.assign((size_t)s, E(1));
        if (counted) count.assign((size_t)s, 0);
    }
    void span(int64_t i, int width) const {
        if (i < 0 || i + width > size) die(name, i, size);
        if (width > 1 && (addr + sizeof(E) * (uint64_t)i) % (sizeof(E) * width)) die("misaligned vector access", i, size);
    }
    E ld(int64_t i, int width = 1) {
        span(i, width);
        g_accesses += width;
        E v = E(0);
        if (!real.empty())
            for (int k = 0; k < width; ++k) v += real.data()[i + k];  // a raw read: the sanitizer sees it
        return v;
    }
    void st(int64_t i, E v, int width = 1) {
        span(i, width);
        g_accesses += width;
        for (int k = 0; k < width; ++k) {
            if (!real.empty()) real.data()[i + k] = v;
            if (!count.empty() && ++count[(size_t)(i + k)] != 1) die("written twice", i + k, size);
        }
    }
    void all_written() const {
        for (int64_t i = 0; i < size; ++i)
            if (count[(size_t)i] != 1) die("not written", i, size);
    }
};

struct Shape {
    int64_t B;
    int obs, pred, J;
    int64_t total_frames;
};

// load_span: n floats of global `src` from element g0 into LDS `dst` from element l0
void load_span(Buf<float>& src, int64_t g0, int N, Buf<float>& dst, int l0, int64_t lo, int64_t hi) {
    int head, quads;
    span_split(src.addr + 4 * (uint64_t)g0, N, head, quads);
    if (head < 0 || quads < 0 || head + 4 * quads > N) die("span split", head + 4 * quads, N);
    if (g0 < lo || g0 + N > hi) die("tile outside the segment's block", g0, hi);
    for (int tid = 0; tid < kThreads; ++tid) {
        for (int e = tid; e < head; e += kThreads) dst.st(l0 + e, src.ld(g0 + e));
        for (int q = tid; q < quads; q += kThreads) {
            const float v = src.ld(g0 + head + 4 * q, 4);
            for (int k = 0; k < 4; ++k) dst.st(l0 + head + 4 * q + k, v);
        }
        for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst.st(l0 + e, src.ld(g0 + e));
    }
}

// store_span: N floats of LDS `src` from element l0 to global `dst` from element g0
void store_span(Buf<float>& dst, int64_t g0, Buf<float>& src, int l0, int N) {
    int head, quads;
    span_split(dst.addr + 4 * (uint64_t)g0, N, head, quads);
    if (head < 0 || quads < 0 || head + 4 * quads > N) die("span split", head + 4 * quads, N);
    for (int tid = 0; tid < kThreads; ++tid) {
        for (int e = tid; e < head; e += kThreads) dst.st(g0 + e, src.ld(l0 + e));
        for (int q = tid; q < quads; q += kThreads) {
            float v = 0.f;
            for (int k = 0; k < 4; ++k) v += src.ld(l0 + head + 4 * q + k);
            dst.st(g0 + head + 4 * q, v, 4);
        }
        for (int e = head + 4 * quads + tid; e < N; e += kThreads) dst.st(g0 + e, src.ld(l0 + e));
    }
}

// frames_phase / out_phase: the 16-byte phase (in floats) of the frames base and of the obs / pred bases
void emulate(const Shape& s, bool real, int frames_phase, int out_phase, bool noisy) {
    const int J = s.J, seg_len = s.obs + s.pred, TF = frame_tile(J), nt = tiles(seg_len, J);
    if (TF * 3 * J > kStageFloats || TF < 1) die("tile exceeds the stage", TF * 3 * J, kStageFloats);
    if (s.total_frames < seg_len) die("total_frames", s.total_frames, seg_len);
    const int64_t nseg = s.total_frames - seg_len + 1;  // every possible start, the last one included
    Buf<float> frames("frames", s.total_frames * 3 * J, real, 0x10000 + 4 * (uint64_t)frames_phase);
    Buf<int64_t> seg_first("seg_first", nseg, real), sample_idx("sample_idx", s.B, real);
    Buf<float> obs("obs", s.B * s.obs * 3 * (J - 1), real, 0x20000 + 4 * (uint64_t)out_phase, true);
    Buf<float> pred("pred", s.B * s.pred * 3 * (J - 1), real, 0x30000 + 4 * (uint64_t)((out_phase + 1) & 3), true);
    Buf<int64_t> segment_idx("segment_idx", s.B, real, 0x10000, true);
    Buf<int32_t> d_offset("draw_offset", s.B, real), d_degrees("draw_degrees", s.B, real);
    Buf<uint8_t> d_mirror("draw_mirror", 2 * s.B, real), d_mask("draw_noise_mask", s.B * s.obs * (J - 1), real);
    Buf<float> d_noise("draw_noise", s.B * s.obs * (J - 1) * 3, real), rot("rot_table", 720, real);

    // ---- k_motion_batch: grid B * tiles ----
    const int64_t grid = s.B * nt;
    if (grid > INT32_MAX) die("grid", grid, INT32_MAX);
    for (int64_t wg = 0; wg < grid; ++wg) {
        const int64_t b = wg / nt;
        const int tile = (int)(wg - b * nt);
        Buf<float> raw("raw (LDS)", kStageFloats, real), outb("outb (LDS)", kStageFloats, real);
        // thread 0: the decisions and the segment.  Sample indices sweep the table and overshoot it at both
        // ends (the clamp); the table's entries overshoot the frames at both ends (clamp_first)
        sample_idx.ld(b);
        d_offset.ld(b);
        d_mirror.ld(2 * b);
        d_mirror.ld(2 * b + 1);
        d_degrees.ld(b);
        const int64_t sidx = (b % 3 == 0) ? -5 + b : (b % 3 == 1 ? nseg - 1 - b / 3 : nseg + 7);
        const int64_t seg = segment_index(sidx, 1, 2, (b % 5) - 2, nseg);
        seg_first.ld(seg);
        const int64_t table = (b % 7 == 3) ? s.total_frames : (b % 7 == 5 ? -3 : seg);  // a corrupt table entry now and then
        const int64_t first = clamp_first(table, s.total_frames, seg_len);
        if (tile == 0) segment_idx.st(b, seg);
        const int t0 = tile * TF, n = TF < seg_len - t0 ? TF : seg_len - t0;
        if (n < 1) die("empty tile", n, 1);
        load_span(frames, raw_frame(first, J, t0), n * 3 * J, raw, 0, raw_frame(first, J, 0), raw_frame(first, J, seg_len));
        rot.ld(b % 360);
        rot.ld(360 + b % 360);
        for (int tid = 0; tid < kThreads; ++tid)
            for (int i = tid; i < n * (J - 1); i += kThreads) {
                const int tl = i / (J - 1), j = 1 + (i - tl * (J - 1)), t = t0 + tl;
                if (j < 1 || j >= J || tl >= n) die("joint / frame", j, J);
                for (int c = 0; c < 3; ++c) {
                    raw.ld(lds_raw(J, tl) + 3 * j + c);
                    raw.ld(lds_raw(J, tl) + c);
                }
                if (noisy && t < s.obs) {
                    const int64_t p = noise_pair(b, s.obs, J, t, j);
                    d_mask.ld(p);
                    for (int c = 0; c < 3; ++c) d_noise.ld(3 * p + c);
                    const uint32_t q = noise_quad(J, t, j);
                    if (q < kQuadNoise0 || q >= kQuadNoise0 + (uint32_t)(s.obs * (J - 1))) die("noise quad", q, s.obs * (J - 1));
                }
                for (int c = 0; c < 3; ++c) outb.st(lds_out(J, tl) + 3 * (j - 1) + c, 1.f);
            }
        const int n_obs = obs_frames_in_tile(t0, n, s.obs);
        if (n_obs < 0 || n_obs > n) die("obs frames in tile", n_obs, n);
        if (n_obs > 0) store_span(obs, out_frame(b, s.obs, J, t0), outb, lds_out(J, 0), n_obs * 3 * (J - 1));
        if (n_obs < n) {
            const int tp = t0 + n_obs - s.obs;
            if (tp < 0 || tp + (n - n_obs) > s.pred) die("pred frame", tp, s.pred);
            store_span(pred, out_frame(b, s.pred, J, tp), outb, lds_out(J, n_obs), (n - n_obs) * 3 * (J - 1));
        }
    }
    obs.all_written();
    pred.all_written();
    segment_idx.all_written();

    // ---- k_motion_draws: grid B ----
    Buf<int32_t> o_offset("offset", s.B, real, 0x10000, true), o_degrees("degrees", s.B, real, 0x10000, true);
    Buf<uint8_t> o_mirror("mirror", 2 * s.B, real, 0x10000, true), o_mask("noise_mask", s.B * s.obs * (J - 1), real, 0x10000, true);
    Buf<float> o_noise("noise", s.B * s.obs * (J - 1) * 3, real, 0x10000, true);
    for (int64_t b = 0; b < s.B; ++b) {
        sample_idx.ld(b);
        o_offset.st(b, 0);
        o_mirror.st(2 * b, 0);
        o_mirror.st(2 * b + 1, 0);
        o_degrees.st(b, 0);
        for (int tid = 0; tid < kThreads; ++tid)
            for (int i = tid; i < s.obs * (J - 1); i += kThreads) {
                const int t = i / (J - 1), j = 1 + (i - t * (J - 1));
                const int64_t p = noise_pair(b, s.obs, J, t, j);
                o_mask.st(p, 0);
                for (int c = 0; c < 3; ++c) o_noise.st(3 * p + c, 0.f);
            }
    }
    o_offset.all_written();
    o_mirror.all_written();
    o_degrees.all_written();
    o_mask.all_written();
    o_noise.all_written();
}

}  // namespace

int main() {
    // the fixture's shapes (obs 5, pred 7 over 130 frames at J = 17, 22, 52) and the shape edges of
    // tests/test_gpu_motion_batch.py (B = 1, obs 1, a tile larger than the segment, a segment one frame longer
    // than a tile, J = 2 and 64) on real buffers, the inputs and outputs at each of the four 16-byte phases
    const Shape small[] = {
        {31, 5, 7, 17, 130}, {31, 5, 7, 22, 130}, {31, 5, 7, 52, 130}, {94, 5, 7, 17, 130}, {1, 5, 7, 17, 12},
        {3, 1, 7, 17, 40},   {5, 2, 3, 17, 9},    {4, 20, 13, 17, 50}, {4, 9, 5, 52, 30},   {3, 6, 5, 64, 20},
        {3, 40, 33, 2, 90},  {2, 33, 40, 2, 80},  {2, 11, 1, 64, 14},  {7, 3, 29, 21, 64},
    };
    for (const Shape& s : small)
        for (int phase = 0; phase < 4; ++phase) {
            emulate(s, true, phase, (phase * 3 + 1) & 3, true);
            emulate(s, true, phase, phase, false);
        }
    // the training and evaluation shapes, indices checked arithmetically
    emulate({1024, 25, 100, 17, 450000}, false, 0, 0, true);
    emulate({1024, 25, 100, 17, 450000}, false, 3, 1, true);
    emulate({512, 30, 120, 52, 450000}, false, 0, 0, true);
    emulate({512, 30, 120, 52, 450000}, false, 1, 2, true);
    std::printf("motion batch emulation ok: %lld accesses in bounds\n", g_accesses);
    return 0;
}
