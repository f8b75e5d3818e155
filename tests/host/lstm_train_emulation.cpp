// Stand-alone host check of the graph-LSTM training core's shared text (csrc/sd_lstm_gates.h with
// the index arithmetic of sd_gru_gates.h): the gate forward / backward formulas restated over heap
// buffers in double in the kernels' own decomposition (per-step P_t = a_t + W_hh h_{t-1} + b_hh, the
// gate record [i | f | g | o], the kept cell states, dQ, dP = gx^T dQ, the carries through h and s,
// batched da / dgx / dW / db with h_{t-1} read from h0 / hs) and compared with central finite
// differences of the same forward.  Built with -fsanitize=address,undefined by
// tests/test_lstm_train_host.py: an index that strays leaves the buffers.  Prints
// "lstm train emulation ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../skeletondiffusion_amd/csrc/sd_lstm_gates.h"

using namespace sd::lstm;
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
    vec a, h0, s0, gx, W, b;
    std::vector<int> type;
};

struct State {
    vec hs, P, gates, sseq;
};

// h_{t-1} of (row b, node j): h0 at the first step, hs otherwise (k_lstm_hh's hp / k_lstm_hprev)
static const double* hprev_of(const Shape& s, const Inputs& in, const State& st, int b, int t, int j) {
    return t == 0 ? &in.h0[((size_t)b * s.J + j) * s.H] : &st.hs[at4(b, t - 1, j, s.T, s.J, s.H)];
}

static void forward(const Shape& s, const Inputs& in, State& st) {
    const int J = s.J, H = s.H, H4 = 4 * H, T = s.T;
    st.hs.assign((size_t)s.B * T * J * H, 0.0);
    st.sseq.assign((size_t)s.B * T * J * H, 0.0);
    st.P.assign((size_t)s.B * T * J * H4, 0.0);
    st.gates.assign((size_t)s.B * T * J * H4, 0.0);
    vec Q(J * H4);
    for (int b = 0; b < s.B; ++b)
        for (int t = 0; t < T; ++t) {
            for (int j = 0; j < J; ++j) {  // k_lstm_hh
                const int ty = in.type[j];
                const double* hp = hprev_of(s, in, st, b, t, j);
                for (int n = 0; n < H4; ++n) {
                    double acc = s.bias ? in.b[(size_t)ty * H4 + n] : 0.0;
                    for (int k = 0; k < H; ++k) acc += in.W[((size_t)ty * H4 + n) * H + k] * hp[k];
                    st.P[at4(b, t, j, T, J, H4) + n] = in.a[at4(b, step_of(t, s.Ta), j, s.Ta, J, H4) + n] + acc;
                }
            }
            const double* g = &in.gx[(size_t)step_of(t, s.Tg) * J * J];
            for (int i = 0; i < J; ++i)  // k_lstm_gate
                for (int n = 0; n < H4; ++n) {
                    double q = 0;
                    for (int j = 0; j < J; ++j) q += g[i * J + j] * st.P[at4(b, t, j, T, J, H4) + n];
                    Q[i * H4 + n] = q;
                }
            for (int i = 0; i < J; ++i)
                for (int k = 0; k < H; ++k) {
                    const double* q = &Q[i * H4];
                    const double sprev =
                        t == 0 ? in.s0[((size_t)b * J + i) * H + k] : st.sseq[at4(b, t - 1, i, T, J, H) + k];
                    const GateFwd<double> f = gate_forward(q[k], q[H + k], q[2 * H + k], q[3 * H + k], sprev);
                    st.hs[at4(b, t, i, T, J, H) + k] = f.h;
                    st.sseq[at4(b, t, i, T, J, H) + k] = f.s;
                    double* gp = &st.gates[at4(b, t, i, T, J, H4) + k];
                    gp[0] = f.i;
                    gp[H] = f.f;
                    gp[2 * H] = f.g;
                    gp[3 * H] = f.o;
                }
        }
}

struct Grads {
    vec da, dh0, ds0, dgx, dW, db;
};

static void backward(const Shape& s, const Inputs& in, const State& st, const vec& dhs, Grads& g) {
    const int J = s.J, H = s.H, H4 = 4 * H, T = s.T, B = s.B, nt = s.types > 0 ? s.types : 1;
    vec dQ((size_t)B * T * J * H4, 0.0), dP((size_t)B * T * J * H4, 0.0);
    vec cs((size_t)B * J * H, 0.0), dhc((size_t)B * J * H, 0.0);
    for (int t = T - 1; t >= 0; --t) {
        const double* gx = &in.gx[(size_t)step_of(t, s.Tg) * J * J];
        const bool first = t == T - 1;
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < J; ++i)
                for (int k = 0; k < H; ++k) {  // k_lstm_gate_bwd
                    const size_t e = ((size_t)b * J + i) * H + k;
                    const int64_t JH = (int64_t)J * H;
                    const int64_t o1 = at4(b, t, i, T, J, H) + k, o4 = at4(b, t, i, T, J, H4) + k;
                    const double dh = dhs[o1] + (first ? 0.0 : dhc[e]);
                    const double sprev = t == 0 ? in.s0[e] : st.sseq[o1 - JH];
                    const GateBwd<double> q =
                        gate_backward(dh, first ? 0.0 : cs[e], st.gates[o4], st.gates[o4 + H], st.gates[o4 + 2 * H],
                                      st.gates[o4 + 3 * H], st.sseq[o1], sprev);
                    dQ[o4] = q.qi;
                    dQ[o4 + H] = q.qf;
                    dQ[o4 + 2 * H] = q.qg;
                    dQ[o4 + 3 * H] = q.qo;
                    cs[e] = q.carry;
                }
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < J; ++j) {  // k_lstm_bwd_hh
                for (int n = 0; n < H4; ++n) {
                    double acc = 0;
                    for (int i = 0; i < J; ++i) acc += gx[i * J + j] * dQ[at4(b, t, i, T, J, H4) + n];
                    dP[at4(b, t, j, T, J, H4) + n] = acc;
                }
                for (int k = 0; k < H; ++k) {
                    double acc = 0;
                    for (int n = 0; n < H4; ++n)
                        acc += in.W[((size_t)in.type[j] * H4 + n) * H + k] * dP[at4(b, t, j, T, J, H4) + n];
                    dhc[((size_t)b * J + j) * H + k] = acc;
                }
            }
    }
    g.dh0 = dhc;
    g.ds0 = cs;
    g.da.assign((size_t)B * s.Ta * J * H4, 0.0);
    g.dgx.assign((size_t)s.Tg * J * J, 0.0);
    g.dW.assign((size_t)nt * H4 * H, 0.0);
    g.db.assign((size_t)nt * H4, 0.0);
    const int64_t n_row = (int64_t)J * H4;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            for (int64_t k = 0; k < n_row; ++k)  // k_lstm_da: a copy (Ta = T) or the sum over the steps in order
                g.da[((int64_t)b * s.Ta + step_of(t, s.Ta)) * n_row + k] += dP[((int64_t)b * T + t) * n_row + k];
            for (int i = 0; i < J; ++i)
                for (int j = 0; j < J; ++j) {  // k_lstm_dgx_part
                    double acc = 0;
                    for (int n = 0; n < H4; ++n)
                        acc += dQ[at4(b, t, i, T, J, H4) + n] * st.P[at4(b, t, j, T, J, H4) + n];
                    g.dgx[(size_t)step_of(t, s.Tg) * J * J + i * J + j] += acc;
                }
            for (int j = 0; j < J; ++j) {  // dW_hh, db_hh over all B T rows, x = h_{t-1}
                const double* hp = hprev_of(s, in, st, b, t, j);
                for (int n = 0; n < H4; ++n) {
                    const double d = dP[at4(b, t, j, T, J, H4) + n];
                    g.db[(size_t)in.type[j] * H4 + n] += d;
                    for (int k = 0; k < H; ++k) g.dW[((size_t)in.type[j] * H4 + n) * H + k] += d * hp[k];
                }
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
    const int J = s.J, H = s.H, H4 = 4 * H, nt = s.types > 0 ? s.types : 1;
    Inputs in;
    in.a = randv((size_t)s.B * s.Ta * J * H4, 1.5);  // pre-activations well outside the linear range
    in.h0 = randv((size_t)s.B * J * H, 0.8);
    in.s0 = randv((size_t)s.B * J * H, 1.2);
    in.gx = randv((size_t)s.Tg * J * J, 1.0 / J * 2.0);
    for (int t = 0; t < s.Tg; ++t)
        for (int i = 0; i < J; ++i) in.gx[((size_t)t * J + i) * J + i] += 0.7;
    in.W = randv((size_t)nt * H4 * H, 1.0 / sqrt((double)H));
    in.b = randv((size_t)nt * H4, 0.3);
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
    } sets[] = {{"da", &in.a, &g.da},    {"dh0", &in.h0, &g.dh0},  {"ds0", &in.s0, &g.ds0},
                {"dgx", &in.gx, &g.dgx}, {"dW_hh", &in.W, &g.dW}, {"db_hh", &in.b, &g.db}};
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

int main() {
    // the smallest shapes of tests/test_gpu_lstm_train.py, every Ta / Tg combination, typed weights
    // with repeated types and shared weights, with and without bias
    const Shape shapes[] = {
        {21, 96, 1, 1, 1, 1, 5, true},  {17, 32, 37, 2, 2, 1, 0, true}, {17, 32, 3, 2, 1, 2, 4, false},
        {3, 16, 2, 4, 4, 4, 2, true},   {5, 16, 2, 3, 1, 1, 0, false},  {16, 16, 2, 3, 3, 1, 16, true},
        {4, 16, 2, 5, 1, 5, 3, true},
    };
    for (const Shape& s : shapes) check_core(s);
    if (g_fail) {
        printf("%d mismatches\n", g_fail);
        return 1;
    }
    printf("lstm train emulation ok\n");
    return 0;
}
