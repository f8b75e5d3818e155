// Gate math and index arithmetic of the graph-GRU training core (sd_gru_train.hip), in one
// __host__ __device__ header: the kernels include it, and so does the stand-alone host program
// tests/host/gru_train_emulation.cpp, which checks this very text against finite differences in
// double (recurrent.py:321-366 with clockwork off; notation of sd_decoder.hip's header comment).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_GRU_HD __host__ __device__ inline
#else
#define SD_GRU_HD inline
#endif

namespace sd {
namespace gru {

SD_GRU_HD float exp_(float x) { return expf(x); }
SD_GRU_HD double exp_(double x) { return exp(x); }
SD_GRU_HD float tanh_(float x) { return tanhf(x); }
SD_GRU_HD double tanh_(double x) { return tanh(x); }
SD_GRU_HD float abs_(float x) { return fabsf(x); }
SD_GRU_HD double abs_(double x) { return fabs(x); }

template <class T>
SD_GRU_HD T sigmoid(T x) {
    return T(1) / (T(1) + exp_(-x));
}

// forward of one (row, node, feature): X_* = (gx a)_*, Hh_* = (gx c)_*
//   r = sigma(X_r + Hh_r), z = sigma(X_z + Hh_z), n = tanh(X_n + r Hh_n), h = n - n z + z h_prev
template <class T>
struct GateFwd {
    T r, z, n, h;
};
template <class T>
SD_GRU_HD GateFwd<T> gate_forward(T xr, T xz, T xn, T hr, T hz, T hn, T hprev) {
    GateFwd<T> g;
    g.r = sigmoid(xr + hr);
    g.z = sigmoid(xz + hz);
    g.n = tanh_(xn + g.r * hn);
    g.h = g.n - g.n * g.z + g.z * hprev;
    return g;
}

// backward of the same element from dh, the gradient arriving at h:
//   dn = dh (1 - z), dz = dh (h_prev - n), carry = dh z           (the direct path into h_prev)
//   pn = dn (1 - n^2), pr = pn Hh_n r (1 - r), pz = dz z (1 - z)
//   dX = (pr, pz, pn), dHh = (pr, pz, pn r)
template <class T>
struct GateBwd {
    T pr, pz, pn, pnr, carry;
};
template <class T>
SD_GRU_HD GateBwd<T> gate_backward(T dh, T r, T z, T n, T hhn, T hprev) {
    GateBwd<T> g;
    const T dn = dh * (T(1) - z);
    const T dz = dh * (hprev - n);
    g.carry = dh * z;
    g.pn = dn * (T(1) - n * n);
    g.pr = g.pn * hhn * (r * (T(1) - r));
    g.pz = dz * (z * (T(1) - z));
    g.pnr = g.pn * r;
    return g;
}

// y = u / max(sum|u|, eps) over a row (F.normalize(p=1, dim=1)); with nrm = sum|u|, d = max(nrm, eps)
// and dot = sum_k dy_k u_k over the row:  du_j = dy_j / d - [nrm >= eps] sign(u_j) dot / d^2
template <class T>
SD_GRU_HD T l1_den(T nrm, T eps) {
    return nrm > eps ? nrm : eps;
}
template <class T>
SD_GRU_HD T l1_backward(T dy, T u, T dot, T nrm, T eps) {
    const T d = l1_den(nrm, eps);
    const T sg = u > T(0) ? T(1) : (u < T(0) ? T(-1) : T(0));
    return dy / d - (nrm >= eps ? sg * (dot / (d * d)) : T(0));
}

// ---- index arithmetic (element offsets, row-major) -------------------------------------------
// (B, T, J, W) tensors: element (b, t, j, 0)
SD_GRU_HD int64_t at4(int64_t b, int64_t t, int64_t j, int64_t T, int64_t J, int64_t W) {
    return ((b * T + t) * J + j) * W;
}
// gates (B, T, J, 4H) = [r | z | n | Hh_n];  dP (B, T, J, 4H) = [pr | pz | pn | pn r]:
// dX = columns [0, 3H) of dP, dHh column q of 3H = dP column hh_col(q, H)
SD_GRU_HD int hh_col(int q, int H) { return q < 2 * H ? q : q + H; }
// a (B, Ta, J, 3H) with Ta in {1, T}; gx (Tg, J, J) with Tg in {1, T}: the slab step t reads
SD_GRU_HD int64_t step_of(int64_t t, int64_t Tx) { return Tx == 1 ? 0 : t; }

}  // namespace gru
}  // namespace sd
