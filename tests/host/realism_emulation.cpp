// Host emulation of the address arithmetic of sd_realism.hip (k_realism_target, k_realism_pred,
// k_realism_reduce): every workgroup x thread x load / store of the three kernels, with the offsets,
// LDS indices and loop bounds of skeletondiffusion_amd/csrc/sd_realism_addr.h, the same functions the
// kernels call.  Small shapes run on real heap buffers of the exact sizes (build with
// -fsanitize=address,undefined: an access outside one aborts); large shapes check every index against
// the buffer's size arithmetically.  16-byte loads must be 16-byte aligned and stay inside the sample's
// own block.  Built and run by tests/test_realism_host.py; no GPU, nothing preloaded.
//
//   realism_emulation            all built-in shapes
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_realism_addr.h"

using namespace sd::realism;

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

struct Shape {
    int64_t B;
    int S, T, Tt, J, L, P;
};

// joint / limb indices that sweep the whole range, both orders
void tables(const Shape& s, std::vector<int>& la, std::vector<int>& lb, std::vector<int>& pa, std::vector<int>& pb) {
    for (int l = 0; l < s.L; ++l) {
        la.push_back(l % 2 ? s.J - 1 - (l % s.J) : l % s.J);
        lb.push_back(l % 3 ? (l * 7) % s.J : s.J - 1);
    }
    for (int p = 0; p < s.P; ++p) {
        pa.push_back(p % s.L);
        pb.push_back(s.L - 1 - (p % s.L));
    }
}

template <class F>
void frame_joint(F&& ld, int64_t base, int j) {  // the three floats of a joint
    ld(base + 3 * j);
    ld(base + 3 * j + 1);
    ld(base + 3 * j + 2);
}

void emulate(const Shape& s, bool real, int pred_phase, bool angles) {
    const int J3 = 3 * s.J, TF = frame_tile(s.J);
    const int64_t BS = s.B * s.S;
    std::vector<int> la, lb, pa, pb;
    tables(s, la, lb, pa, pb);
    Buf<float> pred("pred", BS * s.T * J3, real, 0x10000 + 4 * (uint64_t)pred_phase);
    Buf<float> target("target", s.B * s.Tt * J3, real);
    Buf<double> gt_len("gt_len", s.B * s.L, real), gt_cos("gt_cos", s.B * s.T * s.P, real),
        gt_ang("gt_ang", s.B * s.T * s.P, real);
    Buf<float> none_out("none_out", kQuantities * BS * s.L, real), ps_out("persample_out", kQuantities * BS, real),
        mean_out("mean_out", kQuantities * s.B, real), ang_ps("angle_persample", BS, real), ang_min("angle_min", s.B, real),
        mscratch("motion_scratch", BS * (s.T - 1), real), motion("motion_out", s.B * (s.T - 1), real);
    Buf<double> scratch("limb_scratch", kQuantities * BS * s.L, real);

    // ---- k_realism_target: grid B ----
    for (int64_t b = 0; b < s.B; ++b) {
        Buf<double> ll("target ll (LDS)", kMaxTile * kMaxLimbs, real);
        auto tg = [&](int64_t i) { target.ld(i); };
        for (int t0 = 0; t0 < s.Tt; t0 += kMaxTile) {
            const int n = kMaxTile < s.Tt - t0 ? kMaxTile : s.Tt - t0;
            for (int tid = 0; tid < kThreads; ++tid)
                for (int i = tid; i < n * s.L; i += kThreads) {
                    const int tl = i / s.L, l = i - tl * s.L;
                    frame_joint(tg, target_frame(b, s.Tt, s.J, t0 + tl), la[l]);
                    frame_joint(tg, target_frame(b, s.Tt, s.J, t0 + tl), lb[l]);
                    ll.st(i, 1.0);
                }
            for (int tid = 0; tid < s.L; ++tid)
                for (int tl = 0; tl < n; ++tl) ll.ld(tl * s.L + tid);
        }
        for (int tid = 0; tid < s.L; ++tid) gt_len.st(gt_len_index(b, s.L, tid), 1.0);
        if (angles)  // needs Tt == T
            for (int tid = 0; tid < kThreads; ++tid)
                for (int i = tid; i < s.T * s.P; i += kThreads) {
                    const int t = i / s.P, p = i - t * s.P;
                    for (int l : {pa[p], pb[p]}) {
                        frame_joint(tg, target_frame(b, s.T, s.J, t), la[l]);
                        frame_joint(tg, target_frame(b, s.T, s.J, t), lb[l]);
                    }
                    gt_cos.st(gt_pair_index(b, s.T, t, s.P, p), 1.0);
                    gt_ang.st(gt_pair_index(b, s.T, t, s.P, p), 1.0);
                }
    }

    // ---- k_realism_pred: grid B * S, dynamic LDS lds_bytes(J, L) ----
    if (lds_bytes(s.J, s.L) > 64 * 1024) die("dynamic LDS bytes", (int64_t)lds_bytes(s.J, s.L), 64 * 1024);
    for (int64_t w = 0; w < BS; ++w) {
        const int64_t b = w / s.S;
        Buf<double> ll("ll (LDS)", lds_ll_doubles(s.J, s.L), real);
        Buf<float> fr("frames (LDS)", lds_frame_floats(s.J), real), mb("motion (LDS)", lds_motion_floats(s.J), real);
        auto frl = [&](int64_t i) { fr.ld(i); };
        for (int tid = 0; tid < s.L; ++tid) gt_len.ld(gt_len_index(b, s.L, tid));
        for (int t0 = 0; t0 < s.T; t0 += TF) {
            const int n = TF < s.T - t0 ? TF : s.T - t0;
            const int64_t src = pred_frame(w, s.T, s.J, t0), block0 = pred_frame(w, s.T, s.J, 0),
                          block1 = block0 + (int64_t)s.T * J3;
            const int N = n * J3, dst = lds_slot(s.J, 1);
            int head, quads;
            stage_split(pred.addr + 4 * (uint64_t)src, N, head, quads);
            if (head < 0 || quads < 0 || head + 4 * quads > N) die("stage split", head + 4 * quads, N);
            if (src < block0 || src + N > block1) die("tile outside the sample's block", src, block1);
            for (int tid = 0; tid < kThreads; ++tid) {
                for (int e = tid; e < head; e += kThreads) fr.st(dst + e, pred.ld(src + e));
                for (int q = tid; q < quads; q += kThreads) {
                    const float v = pred.ld(src + head + 4 * q, 4);
                    for (int k = 0; k < 4; ++k) fr.st(dst + head + 4 * q + k, v);
                }
                for (int e = head + 4 * quads + tid; e < N; e += kThreads) fr.st(dst + e, pred.ld(src + e));
            }
            for (int tid = 0; tid < kThreads; ++tid) {
                for (int i = tid; i < n * s.L; i += kThreads) {
                    const int tl = i / s.L, l = i - tl * s.L;
                    frame_joint(frl, lds_slot(s.J, tl + 1), la[l]);
                    frame_joint(frl, lds_slot(s.J, tl + 1), lb[l]);
                    ll.st(i, 1.0);
                }
                for (int i = tid; i < n * s.J; i += kThreads) {
                    const int tl = i / s.J, j = i - tl * s.J;
                    if (t0 + tl == 0) continue;
                    frame_joint(frl, lds_slot(s.J, tl + 1), j);
                    frame_joint(frl, lds_slot(s.J, tl), j);
                    mb.st(i, 1.f);
                }
                if (angles)
                    for (int i = tid; i < n * s.P; i += kThreads) {
                        const int tl = i / s.P, p = i - tl * s.P;
                        for (int l : {pa[p], pb[p]}) {
                            frame_joint(frl, lds_slot(s.J, tl + 1), la[l]);
                            frame_joint(frl, lds_slot(s.J, tl + 1), lb[l]);
                        }
                        gt_cos.ld(gt_pair_index(b, s.T, t0 + tl, s.P, p));
                        gt_ang.ld(gt_pair_index(b, s.T, t0 + tl, s.P, p));
                    }
            }
            if (kMotionLane0 < s.L || kMotionLane0 + n > kCarryLane0) die("thread roles overlap", n, kCarryLane0);
            for (int tid = 0; tid < kThreads; ++tid) {
                if (tid < s.L) {
                    for (int tl = 0; tl < n; ++tl) ll.ld(tl * s.L + tid);
                } else if (tid >= kMotionLane0 && tid < kMotionLane0 + n) {
                    const int tl = tid - kMotionLane0, t = t0 + tl;
                    if (t > 0) {
                        for (int j = 0; j < s.J; ++j) mb.ld(tl * s.J + j);
                        mscratch.st(motion_index(w, s.T, t), 1.f);
                    }
                } else if (tid >= kCarryLane0) {
                    for (int e = tid - kCarryLane0; e < J3; e += kThreads - kCarryLane0)
                        fr.st(lds_slot(s.J, 0) + e, fr.ld(lds_slot(s.J, n) + e));
                }
            }
        }
        for (int tid = 0; tid < s.L; ++tid)
            for (int q = 0; q < kQuantities; ++q) {
                none_out.st(limb_index(q, BS, w, s.L, tid), 1.f);
                scratch.st(limb_index(q, BS, w, s.L, tid), 1.0);
            }
        for (int tid = 0; tid < kQuantities; ++tid) ps_out.st(persample_index(tid, BS, w), 1.f);
        if (angles) ang_ps.st(w, 1.f);
    }

    // ---- k_realism_reduce: grid B ----
    for (int64_t b = 0; b < s.B; ++b) {
        for (int tid = 0; tid < kThreads; ++tid)
            for (int i = tid; i < kQuantities * s.S; i += kThreads) {
                const int q = i / s.S, sm = i - q * s.S;
                if (q * kMaxSamples + sm >= kQuantities * kMaxSamples) die("rows (LDS)", q * kMaxSamples + sm, 0);
                for (int l = 0; l < s.L; ++l) scratch.ld(limb_index(q, BS, b * s.S + sm, s.L, l));
            }
        for (int tid = 0; tid < kQuantities; ++tid) mean_out.st(mean_index(tid, s.B, b), 1.f);
        if (angles) {
            for (int sm = 0; sm < s.S; ++sm) ang_ps.ld(b * s.S + sm);
            ang_min.st(b, 1.f);
        }
        for (int tid = 0; tid < kThreads; ++tid)
            for (int t = 1 + tid; t < s.T; t += kThreads) {
                for (int sm = 0; sm < s.S; ++sm) mscratch.ld(motion_index(b * s.S + sm, s.T, t));
                motion.st(motion_index(b, s.T, t), 1.f);
            }
    }
}

}  // namespace

int main() {
    // the fixture's shapes (tests/test_metrics_realism.py:_cases, the T = 2 / T = 1 edges, the 10-frame
    // observation as target) on real buffers, pred at each of the four 16-byte phases
    const Shape small[] = {
        {2, 7, 20, 20, 16, 16, 12}, {2, 5, 33, 33, 21, 21, 19}, {1, 3, 4, 4, 51, 51, 19}, {1, 2, 5, 5, 17, 17, 14},
        {2, 7, 2, 2, 16, 16, 12},   {2, 7, 1, 1, 16, 16, 12},   {1, 2, 67, 67, 64, 64, 64}, {1, 64, 27, 27, 51, 51, 19},
        {1, 1, 65, 65, 1, 1, 1},
    };
    for (const Shape& s : small)
        for (int phase = 0; phase < 4; ++phase) emulate(s, true, phase, true);
    emulate({2, 7, 20, 10, 16, 16, 0}, true, 1, false);  // obs_as_target: a 10-frame target, no angles
    // the evaluation's shapes, indices checked arithmetically
    emulate({8, 50, 120, 120, 21, 21, 19}, false, 0, true);
    emulate({8, 50, 120, 120, 21, 21, 19}, false, 3, true);
    emulate({256, 50, 120, 120, 21, 21, 19}, false, 0, true);
    std::printf("realism emulation ok: %lld accesses in bounds\n", g_accesses);
    return 0;
}
