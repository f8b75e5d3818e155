// Stand-alone host check of the graph-GRU training core's shared text (csrc/sd_gru_gates.h): the
// gate forward / backward formulas, the L1-normalise backward and the index arithmetic
// (at4 / hh_col / step_of), restated over heap buffers in double in the kernels' own decomposition
// (per-step c_t, gate record [r | z | n | Hh_n], dP = [pr | pz | pn | pn r], dc, batched da / dgx /
// dW / db) and compared with central finite differences of the same forward.  Built with
// -fsanitize=address,undefined by tests/test_gru_train_host.py: an index helper that strays leaves
// the buffers.  Prints "gru train emulation ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_gru_gates.h"

using namespace sd::gru;
typedef std::vector<double> vec;

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double rnd() {  // xorshift, uniform in (-1, 1)
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / (double)(1ull << 53) * 2.0 - 1.0;
}
static vec randv(size_t n, double s) {
    vec v(n);
    for (auto& x : v) x = rnd() * s;
    return v;
}

struct Shape {
    int J, H, B, T, Ta, Tg, types;  // types 0: shared weights
    bool bias;
};

struct Inputs {
    vec a, h0, gx, W, b;
    std::vector<int> type;
};

struct State {
    vec hs, hprev, c, gates;
};

static void forward(const Shape& s, const Inputs& in, State& st) {
    const int J = s.J, H = s.H, H3 = 3 * H, T = s.T;
    st.hs.assign((size_t)s.B * T * J * H, 0.0);
    st.hprev.assign((size_t)s.B * T * J * H, 0.0);
    st.c.assign((size_t)s.B * T * J * H3, 0.0);
    st.gates.assign((size_t)s.B * T * J * 4 * H, 0.0);
    vec X(J * H3), Hh(J * H3);
    for (int b = 0; b < s.B; ++b)
        for (int t = 0; t < T; ++t) {
            for (int j = 0; j < J; ++j)
                for (int k = 0; k < H; ++k)
                    st.hprev[at4(b, t, j, T, J, H) + k] =
                        t == 0 ? in.h0[((size_t)b * J + j) * H + k] : st.hs[at4(b, t - 1, j, T, J, H) + k];
            for (int j = 0; j < J; ++j) {
                const int ty = in.type[j];
                for (int n = 0; n < H3; ++n) {
                    double acc = s.bias ? in.b[(size_t)ty * H3 + n] : 0.0;
                    for (int k = 0; k < H; ++k)
                        acc += in.W[((size_t)ty * H3 + n) * H + k] * st.hprev[at4(b, t, j, T, J, H) + k];
                    st.c[at4(b, t, j, T, J, H3) + n] = acc;
                }
            }
            const double* g = &in.gx[(size_t)step_of(t, s.Tg) * J * J];
            for (int i = 0; i < J; ++i)
                for (int n = 0; n < H3; ++n) {
                    double x = 0, h = 0;
                    for (int j = 0; j < J; ++j) {
                        x += g[i * J + j] * in.a[at4(b, step_of(t, s.Ta), j, s.Ta, J, H3) + n];
                        h += g[i * J + j] * st.c[at4(b, t, j, T, J, H3) + n];
                    }
                    X[i * H3 + n] = x;
                    Hh[i * H3 + n] = h;
                }
            for (int i = 0; i < J; ++i)
                for (int k = 0; k < H; ++k) {
                    const double* x = &X[i * H3];
                    const double* h = &Hh[i * H3];
                    const GateFwd<double> f = gate_forward(x[k], x[H + k], x[2 * H + k], h[k], h[H + k], h[2 * H + k],
                                                           st.hprev[at4(b, t, i, T, J, H) + k]);
                    st.hs[at4(b, t, i, T, J, H) + k] = f.h;
                    double* gp = &st.gates[at4(b, t, i, T, J, 4 * H) + k];
                    gp[0] = f.r;
                    gp[H] = f.z;
                    gp[2 * H] = f.n;
                    gp[3 * H] = h[2 * H + k];
                }
        }
}

struct Grads {
    vec da, dh0, dgx, dW, db;
};

static void backward(const Shape& s, const Inputs& in, const State& st, const vec& dhs, Grads& g) {
    const int J = s.J, H = s.H, H3 = 3 * H, T = s.T, B = s.B, nt = s.types > 0 ? s.types : 1;
    vec dP((size_t)B * T * J * 4 * H, 0.0), dc((size_t)B * T * J * H3, 0.0);
    vec dhz((size_t)B * J * H, 0.0), dhc((size_t)B * J * H, 0.0);
    for (int t = T - 1; t >= 0; --t) {
        const double* gx = &in.gx[(size_t)step_of(t, s.Tg) * J * J];
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < J; ++i)
                for (int k = 0; k < H; ++k) {  // k_gru_gate_bwd
                    const size_t e = ((size_t)b * J + i) * H + k;
                    const int64_t o1 = at4(b, t, i, T, J, H) + k, o4 = at4(b, t, i, T, J, 4 * H) + k;
                    const double dh = dhs[o1] + (t == T - 1 ? 0.0 : dhc[e]);
                    const GateBwd<double> q = gate_backward(dh, st.gates[o4], st.gates[o4 + H], st.gates[o4 + 2 * H],
                                                            st.gates[o4 + 3 * H], st.hprev[o1]);
                    dP[o4] = q.pr;
                    dP[o4 + H] = q.pz;
                    dP[o4 + 2 * H] = q.pn;
                    dP[o4 + 3 * H] = q.pnr;
                    dhz[e] = q.carry;
                }
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < J; ++j) {  // k_gru_bwd_hh
                for (int n = 0; n < H3; ++n) {
                    double acc = 0;
                    for (int i = 0; i < J; ++i) acc += gx[i * J + j] * dP[at4(b, t, i, T, J, 4 * H) + hh_col(n, H)];
                    dc[at4(b, t, j, T, J, H3) + n] = acc;
                }
                for (int k = 0; k < H; ++k) {
                    double acc = dhz[((size_t)b * J + j) * H + k];
                    for (int n = 0; n < H3; ++n)
                        acc += in.W[((size_t)in.type[j] * H3 + n) * H + k] * dc[at4(b, t, j, T, J, H3) + n];
                    dhc[((size_t)b * J + j) * H + k] = acc;
                }
            }
    }
    g.dh0 = dhc;
    g.da.assign((size_t)B * s.Ta * J * H3, 0.0);
    g.dgx.assign((size_t)s.Tg * J * J, 0.0);
    g.dW.assign((size_t)nt * H3 * H, 0.0);
    g.db.assign((size_t)nt * H3, 0.0);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const double* gx = &in.gx[(size_t)step_of(t, s.Tg) * J * J];
            for (int j = 0; j < J; ++j)
                for (int n = 0; n < H3; ++n) {  // k_gru_da
                    double acc = 0;
                    for (int i = 0; i < J; ++i) acc += gx[i * J + j] * dP[at4(b, t, i, T, J, 4 * H) + n];
                    g.da[at4(b, step_of(t, s.Ta), j, s.Ta, J, H3) + n] += acc;
                }
            for (int i = 0; i < J; ++i)
                for (int j = 0; j < J; ++j) {  // k_gru_dgx_part
                    double acc = 0;
                    for (int n = 0; n < H3; ++n) {
                        acc += dP[at4(b, t, i, T, J, 4 * H) + n] * in.a[at4(b, step_of(t, s.Ta), j, s.Ta, J, H3) + n];
                        acc += dP[at4(b, t, i, T, J, 4 * H) + hh_col(n, H)] * st.c[at4(b, t, j, T, J, H3) + n];
                    }
                    g.dgx[(size_t)step_of(t, s.Tg) * J * J + i * J + j] += acc;
                }
            for (int j = 0; j < J; ++j)
                for (int n = 0; n < H3; ++n) {  // dW_hh, db_hh over all B T rows
                    const double d = dc[at4(b, t, j, T, J, H3) + n];
                    g.db[(size_t)in.type[j] * H3 + n] += d;
                    for (int k = 0; k < H; ++k)
                        g.dW[((size_t)in.type[j] * H3 + n) * H + k] += d * st.hprev[at4(b, t, j, T, J, H) + k];
                }
        }
}

static double loss_of(const Shape& s, const Inputs& in, const vec& w) {
    State st;
    forward(s, in, st);
    double l = 0;
    for (size_t i = 0; i < w.size(); ++i) l += w[i] * st.hs[i];
    return l;
}

static int g_fail = 0;
static void compare(const char* what, double an, double fd, double scale) {
    const double err = fabs(an - fd) / scale;
    if (!(err < 1e-6)) {
        printf("MISMATCH %s: analytic %.12g, finite difference %.12g (scale %.3g)\n", what, an, fd, scale);
        ++g_fail;
    }
}

static double maxabs(const vec& v) {
    double m = 0;
    for (double x : v) m = fmax(m, fabs(x));
    return m > 0 ? m : 1.0;
}

static void check_core(const Shape& s) {
    const int J = s.J, H = s.H, H3 = 3 * H, nt = s.types > 0 ? s.types : 1;
    Inputs in;
    in.a = randv((size_t)s.B * s.Ta * J * H3, 0.8);
    in.h0 = randv((size_t)s.B * J * H, 0.8);
    in.gx = randv((size_t)s.Tg * J * J, 1.0 / J * 2.0);
    in.W = randv((size_t)nt * H3 * H, 1.0 / sqrt((double)H));
    in.b = randv((size_t)nt * H3, 0.3);
    in.type.resize(J);
    for (int j = 0; j < J; ++j) in.type[j] = s.types > 0 ? (j * 7 + 3) % s.types : 0;  // repeated types
    const vec w = randv((size_t)s.B * s.T * J * H, 1.0);
    State st;
    forward(s, in, st);
    Grads g;
    backward(s, in, st, w, g);
    struct {
        const char* name;
        vec* x;
        const vec* grad;
    } sets[] = {{"da", &in.a, &g.da}, {"dh0", &in.h0, &g.dh0}, {"dgx", &in.gx, &g.dgx}, {"dW_hh", &in.W, &g.dW},
                {"db_hh", &in.b, &g.db}};
    for (auto& set : sets) {
        if (set.grad == &g.db && !s.bias) continue;
        const double scale = maxabs(*set.grad);
        const size_t n = set.x->size();
        for (int probe = 0; probe < 6; ++probe) {
            const size_t i = probe == 0 ? 0 : (probe == 1 ? n - 1 : (size_t)((rnd() * 0.5 + 0.5) * (n - 1)));
            const double keep = (*set.x)[i], h = 1e-6;
            (*set.x)[i] = keep + h;
            const double lp = loss_of(s, in, w);
            (*set.x)[i] = keep - h;
            const double lm = loss_of(s, in, w);
            (*set.x)[i] = keep;
            compare(set.name, (*set.grad)[i], (lp - lm) / (2 * h), scale);
        }
    }
}

// gx table: gxt[0] = normalize(G) or G, gxt[t + 1] = normalize(gxt[t] + G_add), rows independent
static void gxt_forward(const vec& G, const vec& A, int J, int T, bool norm0, double eps, vec& out) {
    out.assign((size_t)T * J * J, 0.0);
    for (int i = 0; i < J; ++i) {
        vec v(J);
        double s = 0;
        for (int j = 0; j < J; ++j) s += abs_(G[i * J + j]);
        for (int j = 0; j < J; ++j) v[j] = norm0 ? G[i * J + j] / l1_den(s, eps) : G[i * J + j];
        for (int t = 0; t < T; ++t) {
            for (int j = 0; j < J; ++j) out[((size_t)t * J + i) * J + j] = v[j];
            s = 0;
            for (int j = 0; j < J; ++j) {
                v[j] += A[i * J + j];
                s += abs_(v[j]);
            }
            for (int j = 0; j < J; ++j) v[j] /= l1_den(s, eps);
        }
    }
}

static void gxt_backward(const vec& G, const vec& A, const vec& gxt, const vec& dgxt, int J, int T, bool norm0,
                         double eps, vec& dG, vec& dA) {
    dG.assign((size_t)J * J, 0.0);
    dA.assign((size_t)J * J, 0.0);
    for (int i = 0; i < J; ++i) {
        vec g(J), u(J);
        for (int j = 0; j < J; ++j) g[j] = dgxt[((size_t)(T - 1) * J + i) * J + j];
        for (int t = T - 2; t >= -1; --t) {
            if (t == -1 && !norm0) break;
            double nrm = 0, dot = 0;
            for (int j = 0; j < J; ++j) {
                u[j] = t >= 0 ? gxt[((size_t)t * J + i) * J + j] + A[i * J + j] : G[i * J + j];
                nrm += abs_(u[j]);
                dot += g[j] * u[j];
            }
            for (int j = 0; j < J; ++j) {
                const double du = l1_backward(g[j], u[j], dot, nrm, eps);
                if (t >= 0) {
                    dA[i * J + j] += du;
                    g[j] = dgxt[((size_t)t * J + i) * J + j] + du;
                } else {
                    g[j] = du;
                }
            }
        }
        for (int j = 0; j < J; ++j) dG[i * J + j] = g[j];
    }
}

static void check_gxt(int J, int T, bool norm0) {
    const double eps = 1e-12;
    vec G = randv((size_t)J * J, 0.5), A = randv((size_t)J * J, 0.05);
    for (int i = 0; i < J; ++i) G[i * J + i] += 1.0;
    const vec w = randv((size_t)T * J * J, 1.0);
    vec out, dG, dA;
    gxt_forward(G, A, J, T, norm0, eps, out);
    gxt_backward(G, A, out, w, J, T, norm0, eps, dG, dA);
    auto loss = [&]() {
        vec o;
        gxt_forward(G, A, J, T, norm0, eps, o);
        double l = 0;
        for (size_t i = 0; i < o.size(); ++i) l += w[i] * o[i];
        return l;
    };
    struct {
        const char* name;
        vec* x;
        vec* grad;
    } sets[] = {{"gx table dG", &G, &dG}, {"gx table dG_add", &A, &dA}};
    for (auto& set : sets) {
        const double scale = maxabs(*set.grad);
        for (int probe = 0; probe < 8; ++probe) {
            const size_t n = set.x->size(), i = probe == 0 ? 0 : (probe == 1 ? n - 1 : (size_t)((rnd() * 0.5 + 0.5) * (n - 1)));
            const double keep = (*set.x)[i], h = 1e-7;
            (*set.x)[i] = keep + h;
            const double lp = loss();
            (*set.x)[i] = keep - h;
            const double lm = loss();
            (*set.x)[i] = keep;
            compare(set.name, (*set.grad)[i], (lp - lm) / (2 * h), scale);
        }
    }
}

int main() {
    // the smallest shapes of tests/test_gpu_gru_train.py, every Ta / Tg combination, typed weights
    // with repeated types and shared weights, with and without bias
    const Shape shapes[] = {
        {21, 96, 1, 1, 1, 1, 5, true},    {17, 32, 37, 2, 2, 1, 0, true},  {17, 32, 3, 2, 1, 2, 4, false},
        {3, 16, 2, 4, 4, 4, 2, true},     {5, 16, 2, 3, 1, 1, 0, false},   {16, 16, 2, 3, 3, 1, 16, true},
    };
    for (const Shape& s : shapes) check_core(s);
    for (int J : {16, 21})
        for (int T : {1, 2, 30})
            for (bool norm0 : {true, false}) check_gxt(J, T, norm0);
    if (g_fail) {
        printf("%d mismatches\n", g_fail);
        return 1;
    }
    printf("gru train emulation ok\n");
    return 0;
}
