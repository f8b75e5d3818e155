// Gate math of the graph-LSTM training core (sd_lstm_train.hip), in one __host__ __device__
// header: the kernels include it, and so does the stand-alone host program
// tests/host/lstm_train_emulation.cpp, which checks this very text against finite differences in
// double (recurrent.py:126-167 with clockwork off).  Per (row, node, feature), with Q = gx P the
// mixed pre-activations in the chunk order i | f | g | o and s the cell state:
//   i, f, o = sigma(Q_i, Q_f, Q_o), g = tanh(Q_g),  s_t = f s_{t-1} + i g,  h_t = o tanh(s_t)
// The sigmoid / tanh helpers and the index arithmetic are sd_gru_gates.h's.
#pragma once
#include "sd_gru_gates.h"

namespace sd {
namespace lstm {

using gru::at4;
using gru::sigmoid;
using gru::step_of;
using gru::tanh_;

template <class T>
struct GateFwd {
    T i, f, g, o, s, h;
};
template <class T>
SD_GRU_HD GateFwd<T> gate_forward(T qi, T qf, T qg, T qo, T sprev) {
    GateFwd<T> r;
    r.i = sigmoid(qi);
    r.f = sigmoid(qf);
    r.g = tanh_(qg);
    r.o = sigmoid(qo);
    r.s = r.f * sprev + r.i * r.g;
    r.h = r.o * tanh_(r.s);
    return r;
}

// backward of the same element from dh, the gradient arriving at h_t, and carry_s, the gradient
// arriving at s_t from step t + 1:
//   ds = carry_s + dh o (1 - tanh^2 s_t),  carry = ds f                (into s_{t-1})
//   dQ = [ds g i(1-i) | ds s_{t-1} f(1-f) | ds i (1-g^2) | dh tanh(s_t) o(1-o)]
template <class T>
struct GateBwd {
    T qi, qf, qg, qo, carry;
};
template <class T>
SD_GRU_HD GateBwd<T> gate_backward(T dh, T carry_s, T i, T f, T g, T o, T s, T sprev) {
    GateBwd<T> r;
    const T th = tanh_(s);
    const T ds = carry_s + dh * o * (T(1) - th * th);
    r.qi = ds * g * (i * (T(1) - i));
    r.qf = ds * sprev * (f * (T(1) - f));
    r.qg = ds * i * (T(1) - g * g);
    r.qo = dh * th * (o * (T(1) - o));
    r.carry = ds * f;
    return r;
}

}  // namespace lstm
}  // namespace sd
