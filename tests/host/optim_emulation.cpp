// Stand-alone host check of the fused optimizer step, built with
// -fsanitize=address,undefined by tests/test_optim_host.py.  It includes the kernels' own element
// math and chunk arithmetic (csrc/sd_optim_math.h) and the table builder the library launches from
// (csrc/sd_optim_table.h), and restates the kernels' loops over them on the host:
//   * every chunk of every launch is walked as a workgroup walks it (grid stride, 16-byte body,
//     scalar tail) over exactly-sized allocations at 4-, 8- and 16-byte alignment, and every element
//     must be visited exactly once, every partial sum written exactly once;
//   * the float32 update of every variant is compared with a restatement in double.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_optim_math.h"
#include "../../skeletondiffusion_amd/csrc/sd_optim_table.h"

using namespace sd::optim;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("FAILED %s:%d: ", __FILE__, __LINE__);   \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
            exit(1);                                        \
        }                                                   \
    } while (0)

static uint32_t rng_state = 12345u;
static float rnd() {  // uniform in (-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((rng_state >> 8) * (1.0f / 8388608.0f)) - 1.0f;
}

// an array of exactly n floats whose first element sits `align` bytes past a 16-byte boundary
// (align 16: on it), so that AddressSanitizer sees any access past either end
struct Arr {
    void* base = nullptr;
    float* x = nullptr;
    int64_t n = 0;
    void make(int64_t n_, int align) {
        n = n_;
        const size_t lead = (size_t)(align % 16);
        if (posix_memalign(&base, 16, lead + (size_t)n * 4 + (n == 0 && lead == 0 ? 4 : 0)) != 0) exit(2);
        x = (float*)((char*)base + lead);
    }
    ~Arr() { free(base); }
};

struct Tensor {
    Arr p, g, m, v, vmax;
    std::vector<double> dp, dg, dm, dv, dvmax;  // the double restatement's copy
    std::vector<int> visits;
};

static std::vector<int64_t> sizes() {
    std::vector<int64_t> s = {0, 1, 3, 5, 30, 441, kChunk - 1, kChunk, kChunk + 1, 3 * (int64_t)kChunk + 3};
    for (int i = 0; i < kBatch + 5; ++i) s.push_back(7);  // more tensors than one launch carries
    s.push_back(0);
    s.push_back(2);
    return s;
}

// the step kernel's walk (k_opt_step) over one launch with `grid` workgroups
static void walk_step(const OptBatch& b, int grid, float coef, const AdamCall<float>& call, std::vector<Tensor>& ts,
                      const std::vector<int>& slot_tensor) {
    const bool ams = call.flags & kAmsgrad, store_g = call.flags & kStoreGrad;
    const int64_t nchunks = b.first[b.n];
    for (int block = 0; block < grid; ++block)
        for (int64_t c = block; c < nchunks; c += grid) {
            const int t = tensor_of(b.first, b.n, c);
            CHECK(t >= 0 && t < b.n && b.first[t] <= c && c < b.first[t + 1], "chunk %lld -> tensor %d", (long long)c, t);
            const OptTensor& T = b.t[t];
            const int64_t off = (c - b.first[t]) * kChunk;
            const int count = chunk_count(T.numel, off);
            CHECK(count >= 1 && count <= kChunk && off + count <= T.numel, "chunk %lld: off %lld count %d", (long long)c,
                  (long long)off, count);
            float *p = T.p + off, *g = T.g + off, *m = T.m + off, *v = T.v + off, *vm = ams ? T.vmax + off : nullptr;
            const AdamTensor<float> s{T.decay, T.step_size, T.bc2_sqrt};
            const int body =
                vec_body(count, (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vm);
            CHECK(body % 4 == 0 && body <= count, "body %d of %d", body, count);
            if (body) CHECK(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0, "a 16-byte body at an odd address");
            std::vector<int>& visits = ts[(size_t)slot_tensor[(size_t)t]].visits;
            auto one = [&](int i) {
                float P = p[i], G = g[i], M = m[i], V = v[i], X = ams ? vm[i] : 0.f;
                adam_update(P, G, M, V, X, coef, call, s);
                p[i] = P, m[i] = M, v[i] = V;
                if (ams) vm[i] = X;
                if (store_g) g[i] = G;
                ++visits[(size_t)(off + i)];
            };
            for (int tid = 0; tid < kThreads; ++tid) {
                for (int i = tid * 4; i < body; i += kThreads * 4)
                    for (int k = 0; k < 4; ++k) one(i + k);
                for (int i = body + tid; i < count; i += kThreads) one(i);
            }
        }
}

// the norm kernel's walk (k_opt_norm): partial sums in double, one per chunk
static void walk_norm(const OptBatch& b, int grid, std::vector<double>& partials, std::vector<int>& written) {
    const int64_t nchunks = b.first[b.n];
    for (int block = 0; block < grid; ++block)
        for (int64_t c = block; c < nchunks; c += grid) {
            const int t = tensor_of(b.first, b.n, c);
            const int64_t off = (c - b.first[t]) * kChunk;
            const int count = chunk_count(b.t[t].numel, off);
            const float* g = b.t[t].g + off;
            const int body = vec_body(count, (uintptr_t)g);
            double acc = 0.0;
            for (int tid = 0; tid < kThreads; ++tid) {
                for (int i = tid * 4; i < body; i += kThreads * 4)
                    for (int k = 0; k < 4; ++k) acc += (double)g[i + k] * (double)g[i + k];
                for (int i = body + tid; i < count; i += kThreads) acc += (double)g[i] * (double)g[i];
            }
            const int64_t at = b.chunk_base + c;
            CHECK(at >= 0 && at < (int64_t)partials.size(), "partial %lld of %zu", (long long)at, partials.size());
            partials[(size_t)at] = acc;
            ++written[(size_t)at];
        }
}

// the update in double, written out on its own (torch's Adam / AdamW, single-tensor form)
static void step_double(Tensor& t, double coef, bool decoupled, bool amsgrad, double lr, double wd, double beta1,
                        double beta2, double eps, int step) {
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    for (size_t i = 0; i < t.dp.size(); ++i) {
        t.dg[i] *= coef;
        double g = t.dg[i];
        if (decoupled) t.dp[i] *= 1.0 - lr * wd;
        else g += wd * t.dp[i];
        t.dm[i] = beta1 * t.dm[i] + (1.0 - beta1) * g;
        t.dv[i] = beta2 * t.dv[i] + (1.0 - beta2) * g * g;
        double s = t.dv[i];
        if (amsgrad) {
            t.dvmax[i] = fmax(t.dvmax[i], t.dv[i]);
            s = t.dvmax[i];
        }
        t.dp[i] -= (lr / bc1) * t.dm[i] / (sqrt(s) / sqrt(bc2) + eps);
    }
}

struct Pool {
    double err = 0.0, mag = 0.0;
    void add(double x, double ref) {
        err = fmax(err, fabs(x - ref));
        mag = fmax(mag, fabs(ref));
    }
    double rel() const { return mag > 0.0 ? err / mag : err; }
};

static void run_variant(int align, bool decoupled, bool amsgrad, double wd, bool clip, int grid) {
    const std::vector<int64_t> sz = sizes();
    const int n = (int)sz.size();
    std::vector<Tensor> ts((size_t)n);
    for (int i = 0; i < n; ++i) {
        Tensor& t = ts[(size_t)i];
        const int64_t k = sz[(size_t)i];
        t.p.make(k, align), t.g.make(k, align), t.m.make(k, align), t.v.make(k, align), t.vmax.make(k, align);
        t.dp.resize((size_t)k), t.dg.resize((size_t)k), t.dm.assign((size_t)k, 0.0), t.dv.assign((size_t)k, 0.0);
        t.dvmax.assign((size_t)k, 0.0);
        for (int64_t j = 0; j < k; ++j) {
            t.p.x[j] = rnd();
            t.m.x[j] = t.v.x[j] = t.vmax.x[j] = 0.f;
            t.dp[(size_t)j] = t.p.x[j];
        }
    }
    // eps: Adam's quotient m / (sqrt(v) / c + eps) has slope (1 - beta1) / eps in the gradient where the
    // gradient crosses zero, which an L2 term (g + wd p, a sum that cancels) does; at torch's default
    // eps = 1e-8 that slope turns the sum's last-bit error into 1e-5 of p, in torch's float32 as much
    // as here.  This comparison is about the formula, so it runs where the quotient is well
    // conditioned, with eps still the size of sqrt(v) on the first step so that its place is checked.
    const double lr = 1e-2, beta1 = 0.9, beta2 = 0.999, eps = 1e-4, max_norm = 1.0;
    const int flags = (amsgrad ? kAmsgrad : 0) | (decoupled ? kDecoupled : 0) | (clip ? kStoreGrad : 0);
    const AdamCall<float> call{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, flags};
    const float scales[3] = {1e-3f, 1.f, 10.f};  // below max_norm on the first step, above it afterwards
    for (int step = 1; step <= 3; ++step) {
        for (Tensor& t : ts) {
            for (int64_t j = 0; j < t.g.n; ++j) {
                t.g.x[j] = rnd() * scales[step - 1];
                t.dg[(size_t)j] = t.g.x[j];
            }
            t.visits.assign((size_t)t.g.n, 0);
        }
        std::vector<int> slot_tensor;  // launch slot -> tensor, rebuilt per launch below
        std::vector<int> order;
        auto fill = [&](int i, OptTensor* o) {
            Tensor& t = ts[(size_t)i];
            o->p = t.p.x, o->g = t.g.x, o->m = t.m.x, o->v = t.v.x, o->vmax = amsgrad ? t.vmax.x : nullptr;
            o->decay = decoupled ? (float)(1.0 - lr * wd) : (float)wd;
            o->step_size = (float)(lr / (1.0 - pow(beta1, step)));
            o->bc2_sqrt = (float)sqrt(1.0 - pow(beta2, step));
            order.push_back(i);
        };
        const std::vector<OptBatch> batches = build_batches(sz.data(), n, fill);
        const int64_t chunks = total_chunks(sz.data(), n);
        int64_t seen = 0;
        for (const OptBatch& b : batches) {
            CHECK(b.n >= 1 && b.n <= kBatch && b.chunk_base == seen, "launch of %d tensors at chunk %lld", b.n,
                  (long long)b.chunk_base);
            seen += b.first[b.n];
        }
        CHECK(seen == chunks, "launches hold %lld chunks of %lld", (long long)seen, (long long)chunks);
        CHECK(batches.size() >= 2, "the sizes must need more than one launch");

        float coef = 1.f;
        double dcoef = 1.0;
        if (clip) {
            std::vector<double> partials((size_t)chunks, 0.0);
            std::vector<int> written((size_t)chunks, 0);
            for (const OptBatch& b : batches) walk_norm(b, grid, partials, written);
            double sum = 0.0, direct = 0.0;
            for (size_t i = 0; i < partials.size(); ++i) {
                CHECK(written[i] == 1, "partial %zu written %d times", i, written[i]);
                sum += partials[i];
            }
            for (const Tensor& t : ts)
                for (double g : t.dg) direct += g * g;
            CHECK(fabs(sum - direct) <= 1e-12 * direct, "norm^2 %.17g, direct %.17g", sum, direct);
            const float total = (float)sqrt(sum);
            coef = clip_coef(total, (float)max_norm);
            dcoef = clip_coef(sqrt(direct), max_norm);
            CHECK(step == 1 ? coef == 1.f : coef < 1.f, "step %d: coef %g", step, coef);
            CHECK(fabs(coef - dcoef) <= 4e-7 * dcoef, "coef %.9g, in double %.17g", coef, dcoef);
        }
        size_t at = 0;
        for (const OptBatch& b : batches) {
            slot_tensor.assign(order.begin() + (long)at, order.begin() + (long)at + b.n);
            at += (size_t)b.n;
            walk_step(b, grid, coef, call, ts, slot_tensor);
        }
        for (int i = 0; i < n; ++i) {
            for (size_t j = 0; j < ts[(size_t)i].visits.size(); ++j)
                CHECK(ts[(size_t)i].visits[j] == 1, "align %d: element %zu of tensor %d (%lld elements) visited %d times",
                      align, j, i, (long long)sz[(size_t)i], ts[(size_t)i].visits[j]);
            step_double(ts[(size_t)i], dcoef, decoupled, amsgrad, lr, wd, beta1, beta2, eps, step);
        }
    }
    // a clipped gradient of NaN keeps its NaN through the coefficient
    CHECK(clip_coef(NAN, 1.f) != clip_coef(NAN, 1.f), "a NaN norm must give a NaN coefficient");
    Pool pp, pg, pm, pv, px;
    for (const Tensor& t : ts)
        for (int64_t j = 0; j < t.p.n; ++j) {
            pp.add(t.p.x[j], t.dp[(size_t)j]), pm.add(t.m.x[j], t.dm[(size_t)j]), pv.add(t.v.x[j], t.dv[(size_t)j]);
            if (clip) pg.add(t.g.x[j], t.dg[(size_t)j]);
            if (amsgrad) px.add(t.vmax.x[j], t.dvmax[(size_t)j]);
        }
    // three steps of about ten float32 roundings (2^-24 each) on values of magnitude <= the pooled
    // maximum: 1e-5 is thirty times that, and far below any mistake in the formula
    const double tol = 1e-5;
    CHECK(pp.rel() <= tol && pg.rel() <= tol && pm.rel() <= tol && pv.rel() <= tol && px.rel() <= tol,
          "decoupled %d amsgrad %d wd %g clip %d: p %.3g g %.3g m %.3g v %.3g vmax %.3g", decoupled, amsgrad, wd, clip,
          pp.rel(), pg.rel(), pm.rel(), pv.rel(), px.rel());
}

static void check_lerp() {
    for (float w : {0.f, 1.f, 0.005f, 0.25f, 0.5f, 0.9f}) {
        for (int i = 0; i < 1000; ++i) {
            const float a = rnd() * 3.f, b = rnd() * 3.f;
            const float y = lerp2(a, b, w);
            if (w == 0.f) CHECK(y == a, "lerp weight 0");
            if (w == 1.f) CHECK(y == b, "lerp weight 1 must be an exact copy");
            const double r = (double)a + (double)w * ((double)b - (double)a);
            CHECK(fabs(y - r) <= 1e-6 * (fabs((double)a) + fabs((double)b)) + 1e-12, "lerp(%g, %g, %g) = %g, %g", a, b, w, y, r);
        }
    }
}

int main() {
    static_assert(kChunk % (4 * kThreads) == 0, "a chunk is a whole number of 16-byte sweeps");
    int variants = 0;
    for (int align : {4, 8, 16})
        for (int decoupled = 0; decoupled < 2; ++decoupled)
            for (int amsgrad = 0; amsgrad < 2; ++amsgrad)
                for (double wd : {0.0, 0.01})
                    for (int clip = 0; clip < 2; ++clip) {
                        // a grid smaller than the chunk count, so that workgroups stride
                        run_variant(align, decoupled, amsgrad, wd, clip, align == 16 ? 3 : 5);
                        ++variants;
                    }
    check_lerp();
    printf("optim emulation ok (%d variants)\n", variants);
    return 0;
}
