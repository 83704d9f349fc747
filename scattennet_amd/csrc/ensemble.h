// What ensemble.hip (the head ensemble) and distill.hip (the ensemble as the distillation teacher)
// share, so that both form the members' row statistics and the learned weights with one body: the
// by-value member table, the 16-byte / scalar packs, member_stat and ens_device_weights.
#pragma once
#include "ctc.h"

namespace {

constexpr int G_MAX = SCA_EVAL_MAX_HEADS;

// The G row sources and their weights, by value in the kernel arguments (scalar registers).
// x: the head table of the decoders (ctc.h), slots past G filled the same way; w[g] = w_g / sum w;
// lw[g] = log of it ("prob" adds it to the head's log-probabilities).
struct EnsHeads {
  CtcHeads x;
  float w[G_MAX];
  float lw[G_MAX];
};

template <int V>
struct Pack {
  float v[V];
};

template <int V>
__device__ __forceinline__ Pack<V> ldv(const float* p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const f32x4 t = ld4(p);
    r.v[0] = t[0]; r.v[1] = t[1]; r.v[2] = t[2]; r.v[3] = t[3];
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void stv(float* p, const Pack<V>& r) {
  if constexpr (V == 4) {
    f32x4 t;
    t[0] = r.v[0]; t[1] = r.v[1]; t[2] = r.v[2]; t[3] = r.v[3];
    st4(p, t);
  } else {
    *p = r.v[0];
  }
}

// The row statistics of one member's row, by one wave: m = max, ls = log sum exp(x - m).  One
// body under the forward and the backward, so they agree bitwise.
template <int V>
__device__ __forceinline__ void member_stat(const float* __restrict__ xr, int C, int lane, float& m, float& ls) {
  float mx = NEG_INF;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> x = ldv<V>(xr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) mx = fmaxf(mx, x.v[i]);
  }
  mx = wave_max(mx);
  float s = 0.0f;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> x = ldv<V>(xr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) s += __expf(x.v[i] - mx);
  }
  s = wave_sum(s);
  m = mx;
  ls = __logf(s);
}

// The learned ensemble's weights from its G scores theta on the device: W = softmax(theta) and
// lw = log W = (theta - max) - log sum exp(theta - max), W = exp(lw).  Every lane of a wave
// computes all of it once (theta[g] is a wave-uniform load, G <= 8).  One body under the
// forward and the backward, so the backward forms r_g with the forward's own log W_g.
__device__ __forceinline__ void ens_device_weights(const float* __restrict__ theta, int G, float (&w)[G_MAX],
                                                   float (&lw)[G_MAX]) {
  float t[G_MAX];
  float mx = NEG_INF;
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    t[g] = g < G ? theta[g] : NEG_INF;
    mx = fmaxf(mx, t[g]);
  }
  float s = 0.0f;
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < G) s += __expf(t[g] - mx);
  const float ls = __logf(s);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    lw[g] = g < G ? (t[g] - mx) - ls : 0.0f;
    w[g] = g < G ? __expf(lw[g]) : 0.0f;
  }
}

// G normalised weights and their logarithms, in double, for the forward and the backward alike
inline EnsHeads ens_heads_of(const sca_decode_heads* heads, int G, const sca_ensemble_weights* weights, double sum) {
  EnsHeads h;
  h.x = ctc_heads_of(heads, G);
  for (int g = 0; g < G_MAX; ++g) {
    const double w = (double)weights->w[g < G ? g : 0] / sum;
    h.w[g] = (float)w;
    h.lw[g] = (float)log(w);
  }
  return h;
}

}  // namespace
