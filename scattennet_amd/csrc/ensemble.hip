// Ensemble of the recognition heads' posteriors (include/scatten.h, sca_ensemble_log_probs):
// out (B, T, C) = the normalised log-probabilities of the weighted arithmetic ("prob") or
// log-linear ("logprob") mean of G heads' softmax rows.  The multi-stream recognisers decode
// this averaged posterior next to the single heads; in torch it is a log_softmax per head, a
// stack and a logsumexp: G + 2 tensors of (B, T, C) and as many launches.  Here it is one
// launch whatever G is, G reads and one write.
//
// One wave per (b, t) row, four rows per 256-thread workgroup, as the decoders' row pass
// (decode.hip, ctc_rowstat_heads_kernel), and that pass's arithmetic for the row statistics
// (max, then the sum of exp(x - max)).  A row is a few KB, so the second and third reads of it
// come from L2 / L1.  Lanes take 16 bytes each where every head's row and the output row start
// on a 16-byte boundary and C is a multiple of 4; any other row takes the scalar path.
// No atomics, no LDS; every sum runs in a fixed order and a row's result depends on nothing
// but the row, so a replayed capture is bitwise the eager call.
//
// sca_ensemble_log_probs_bwd is the vector-Jacobian product of the same map, one launch for all
// members with the same shape and guarantees; the members' row statistics are recomputed, not
// saved.
//
// sca_ensemble_log_probs_dw / _dw_bwd are the same two maps with learned weights: W = softmax of
// G scores theta that live on the device (ens_device_weights, once per wave), so a captured graph
// follows an optimizer's update of theta.  The row bodies are the ones above, instantiated on
// the weights' source.  d theta is a sum over all rows: every wave stores its row's G partials
// with plain stores and a second launch of one workgroup sums them in a fixed order (DESIGN.md
// §5e.4).
#include "ensemble.h"

namespace {

// One row by one wave; lane l owns the elements [V (l + 64 k), V (l + 64 k) + V) in every pass.
// V = 4 only when C % 4 == 0, so a pack never crosses the end of the row.  h: the members with
// W_g and log W_g, the kernel's arguments (host weights) or filled by ens_device_weights.
template <int V>
__device__ __forceinline__ void ensemble_row(const EnsHeads& h, int G, int mode, long off, float* __restrict__ outr,
                                             int C, int lane) {
  // row statistics of every member: m = max, ls = log sum exp(x - m)
  float m[G_MAX], ls[G_MAX];
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    m[g] = 0.0f;
    ls[g] = 0.0f;
    if (g < G) member_stat<V>(h.x.x[g] + off, C, lane, m[g], ls[g]);
  }

  if (mode == 0) {
    // out[c] = M + log sum_g exp(a_g - M), a_g = lp_g[c] + log w_g, M = max_g a_g: the largest
    // term of the sum is exp(0) = 1, so nothing overflows and the sum never reaches 0
    for (int c = lane * V; c < C; c += 64 * V) {
      float a[G_MAX][V];
      float M[V];
#pragma unroll
      for (int i = 0; i < V; ++i) M[i] = NEG_INF;
#pragma unroll
      for (int g = 0; g < G_MAX; ++g) {
        if (g < G) {
          const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            a[g][i] = ctc_lp_raw(x.v[i], m[g], ls[g]) + h.lw[g];
            M[i] = fmaxf(M[i], a[g][i]);
          }
        }
      }
      Pack<V> o;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < G_MAX; ++g)
          if (g < G) s += __expf(a[g][i] - M[i]);
        o.v[i] = M[i] + __logf(s);
      }
      stv<V>(outr + c, o);
    }
    return;
  }

  // mode 1: u[c] = sum_g w_g lp_g[c] (g ascending), out = u - logsumexp_c u.  u is kept in the
  // output row between the passes: a lane reads back only what it wrote itself.
  float um = NEG_INF;
  for (int c = lane * V; c < C; c += 64 * V) {
    Pack<V> u;
#pragma unroll
    for (int i = 0; i < V; ++i) u.v[i] = 0.0f;
#pragma unroll
    for (int g = 0; g < G_MAX; ++g) {
      if (g < G) {
        const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
#pragma unroll
        for (int i = 0; i < V; ++i) u.v[i] = fmaf(h.w[g], ctc_lp_raw(x.v[i], m[g], ls[g]), u.v[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) um = fmaxf(um, u.v[i]);
    stv<V>(outr + c, u);
  }
  um = wave_max(um);
  float s = 0.0f;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> u = ldv<V>(outr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) s += __expf(u.v[i] - um);
  }
  s = wave_sum(s);
  const float lse = __logf(s);
  for (int c = lane * V; c < C; c += 64 * V) {
    Pack<V> u = ldv<V>(outr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) u.v[i] = (u.v[i] - um) - lse;
    stv<V>(outr + c, u);
  }
}

__global__ __launch_bounds__(256) void ensemble_log_probs_kernel(EnsHeads h, int G, int mode, float* out, long rows,
                                                                 int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;  // no barrier below: a wave without a row leaves
  const long off = row * C;
  float* outr = out + off;
  // 16-byte packs only where every member's row and the output row start on a 16-byte boundary
  uintptr_t bits = reinterpret_cast<uintptr_t>(outr) | (uintptr_t)(C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < G) bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
  if ((bits & 15) == 0)
    ensemble_row<4>(h, G, mode, off, outr, C, lane);
  else
    ensemble_row<1>(h, G, mode, off, outr, C, lane);
}

// The same rows with W = softmax(theta) read from the device: the table is the one above, its
// weights filled here by every wave instead of by the host.
__global__ __launch_bounds__(256) void ensemble_log_probs_dw_kernel(CtcHeads x, const float* __restrict__ theta, int G,
                                                                    int mode, float* out, long rows, int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;  // no barrier below: a wave without a row leaves
  EnsHeads h;
  h.x = x;
  ens_device_weights(theta, G, h.w, h.lw);
  const long off = row * C;
  float* outr = out + off;
  uintptr_t bits = reinterpret_cast<uintptr_t>(outr) | (uintptr_t)(C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < G) bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
  if ((bits & 15) == 0)
    ensemble_row<4>(h, G, mode, off, outr, C, lane);
  else
    ensemble_row<1>(h, G, mode, off, outr, C, lane);
}

// ---- backward: dx_g = (d out / d x_g)^T dout for every member that takes a gradient ----------
// The gradient tensors, by value beside the members.  A null entry: the member takes no
// gradient; nothing of it is computed or written.
struct EnsGrads {
  float* dx[G_MAX];
};

// The row's G partials of d theta, plain stores: lane g < G writes p[g] (the same value in every
// lane after the wave sums).  One predicated store per member: picking p[lane] instead would make
// the register array an indexed one, in scratch.
__device__ __forceinline__ void store_partials(float* __restrict__ pr, const float (&p)[G_MAX], int G, int lane) {
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < G && lane == g) pr[g] = p[g];
}

// One row by one wave, the lanes' elements as in ensemble_row.  q = exp(out), p_g = softmax(x_g).
//   mode 0: r_g[c] = exp(a_g[c] - out[c]), a_g = lp_g + log W_g as the forward computes it (the
//     responsibility of member g for class c, <= 1 up to rounding: nothing overflows);
//     dx_g[k] = r_g[k] dout[k] - p_g[k] sum_c r_g[c] dout[c].  The members' row statistics are
//     recomputed as the forward does (a row is a few KB: the re-reads come from L2 / L1).
//   mode 1: du[c] = dout[c] - q[c] sum_c' dout[c'] and dx_g = W_g du: the term
//     - W_g p_g[k] sum_c du[c] of the chain through log_softmax(x_g) is dropped, the sum being
//     identically 0 (sum q = 1).  The members are not read at all.
// DW (learned weights) and pr, the row's G cells of the partials (null: d theta is not asked
// for): the row's share of d theta, with s_g = sum_c r_g[c] dout[c] and D = sum_c dout[c],
//   mode 0: pr[g] = s_g - W_g D, so s_g is formed for every member, also one with a null dx;
//   mode 1: pr[g] = W_g sum_c du[c] (lp_g[c] - out[c]): out for u is exact because sum_c du = 0.
//     With pr the members and their row statistics are read in this mode too.
// A row with dout = 0 stores G zeros.  Without DW none of this is compiled in.
template <int V, bool DW>
__device__ __forceinline__ void ensemble_bwd_row(const EnsHeads& h, const EnsGrads& d, int G, int mode, long off,
                                                 const float* __restrict__ outr, const float* __restrict__ doutr, int C,
                                                 int lane, [[maybe_unused]] float* __restrict__ pr = nullptr) {
  // member g is read in mode 0: it takes a gradient or, with learned weights, d theta is asked for
  const auto need = [&](int g) {
    if constexpr (DW)
      return g < G && (d.dx[g] || pr);
    else
      return g < G && d.dx[g];
  };
  if (mode == 1) {
    [[maybe_unused]] float m[G_MAX], ls[G_MAX], acc[G_MAX];
    if constexpr (DW) {
#pragma unroll
      for (int g = 0; g < G_MAX; ++g) {
        m[g] = 0.0f;
        ls[g] = 0.0f;
        acc[g] = 0.0f;
        if (pr && g < G) member_stat<V>(h.x.x[g] + off, C, lane, m[g], ls[g]);
      }
    }
    float D = 0.0f;
    for (int c = lane * V; c < C; c += 64 * V) {
      const Pack<V> dy = ldv<V>(doutr + c);
#pragma unroll
      for (int i = 0; i < V; ++i) D += dy.v[i];
    }
    D = wave_sum(D);
    for (int c = lane * V; c < C; c += 64 * V) {
      const Pack<V> o = ldv<V>(outr + c), dy = ldv<V>(doutr + c);
      Pack<V> du;
#pragma unroll
      for (int i = 0; i < V; ++i) du.v[i] = dy.v[i] - __expf(o.v[i]) * D;
#pragma unroll
      for (int g = 0; g < G_MAX; ++g) {
        if (g < G && d.dx[g]) {
          Pack<V> r;
#pragma unroll
          for (int i = 0; i < V; ++i) r.v[i] = h.w[g] * du.v[i];
          stv<V>(d.dx[g] + off + c, r);
        }
      }
      if constexpr (DW) {
        if (pr) {
#pragma unroll
          for (int g = 0; g < G_MAX; ++g) {
            if (g < G) {
              const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
#pragma unroll
              for (int i = 0; i < V; ++i) acc[g] += du.v[i] * (ctc_lp_raw(x.v[i], m[g], ls[g]) - o.v[i]);
            }
          }
        }
      }
    }
    if constexpr (DW) {
      if (pr) {
#pragma unroll
        for (int g = 0; g < G_MAX; ++g)
          if (g < G) acc[g] = h.w[g] * wave_sum(acc[g]);
        store_partials(pr, acc, G, lane);
      }
    }
    return;
  }

  // mode 0.  s[g] = sum_c r_g[c] dout[c], one pass over the classes for all the members
  float m[G_MAX], ls[G_MAX], s[G_MAX];
  [[maybe_unused]] float D = 0.0f;
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    m[g] = 0.0f;
    ls[g] = 0.0f;
    s[g] = 0.0f;
    if (need(g)) member_stat<V>(h.x.x[g] + off, C, lane, m[g], ls[g]);
  }
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> o = ldv<V>(outr + c), dy = ldv<V>(doutr + c);
    if constexpr (DW) {
#pragma unroll
      for (int i = 0; i < V; ++i) D += dy.v[i];
    }
#pragma unroll
    for (int g = 0; g < G_MAX; ++g) {
      if (need(g)) {
        const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float a = ctc_lp_raw(x.v[i], m[g], ls[g]) + h.lw[g];
          s[g] += __expf(a - o.v[i]) * dy.v[i];
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (need(g)) s[g] = wave_sum(s[g]);
  if constexpr (DW) {
    if (pr) {
      D = wave_sum(D);
      float part[G_MAX];
#pragma unroll
      for (int g = 0; g < G_MAX; ++g) part[g] = s[g] - h.w[g] * D;
      store_partials(pr, part, G, lane);
    }
  }
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> o = ldv<V>(outr + c), dy = ldv<V>(doutr + c);
#pragma unroll
    for (int g = 0; g < G_MAX; ++g) {
      if (g < G && d.dx[g]) {
        const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
        Pack<V> r;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float lp = ctc_lp_raw(x.v[i], m[g], ls[g]);
          r.v[i] = __expf((lp + h.lw[g]) - o.v[i]) * dy.v[i] - __expf(lp) * s[g];
        }
        stv<V>(d.dx[g] + off + c, r);
      }
    }
  }
}

__global__ __launch_bounds__(256) void ensemble_log_probs_bwd_kernel(EnsHeads h, EnsGrads d, int G, int mode,
                                                                     const float* out, const float* dout, long rows,
                                                                     int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;  // no barrier below: a wave without a row leaves
  const long off = row * C;
  // 16-byte packs only where every row involved starts on a 16-byte boundary: the members, out,
  // dout and every gradient row that is written
  uintptr_t bits = reinterpret_cast<uintptr_t>(out + off) | reinterpret_cast<uintptr_t>(dout + off) | (uintptr_t)(C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    if (g < G) {
      bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
      if (d.dx[g]) bits |= reinterpret_cast<uintptr_t>(d.dx[g] + off);
    }
  }
  if ((bits & 15) == 0)
    ensemble_bwd_row<4, false>(h, d, G, mode, off, out + off, dout + off, C, lane);
  else
    ensemble_bwd_row<1, false>(h, d, G, mode, off, out + off, dout + off, C, lane);
}

// The same rows with W = softmax(theta) read from the device; part: null, or the (rows, G)
// partials of d theta, of which this wave writes its row's G cells.
__global__ __launch_bounds__(256) void ensemble_log_probs_dw_bwd_kernel(CtcHeads x, EnsGrads d,
                                                                        const float* __restrict__ theta, int G, int mode,
                                                                        const float* out, const float* dout,
                                                                        float* __restrict__ part, long rows, int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;  // no barrier below: a wave without a row leaves
  EnsHeads h;
  h.x = x;
  ens_device_weights(theta, G, h.w, h.lw);
  const long off = row * C;
  float* pr = part ? part + row * G : nullptr;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out + off) | reinterpret_cast<uintptr_t>(dout + off) | (uintptr_t)(C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    if (g < G) {
      bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
      if (d.dx[g]) bits |= reinterpret_cast<uintptr_t>(d.dx[g] + off);
    }
  }
  if ((bits & 15) == 0)
    ensemble_bwd_row<4, true>(h, d, G, mode, off, out + off, dout + off, C, lane, pr);
  else
    ensemble_bwd_row<1, true>(h, d, G, mode, off, out + off, dout + off, C, lane, pr);
}

// d theta (G) = the sum of the (rows, G) partials over the rows, by one workgroup in a fixed
// order: thread t adds the rows t, t + 256, ... ascending, then a tree over the 256 threads in
// LDS.  No atomics: the result depends on the partials alone, so a replay is bitwise the eager call.
__global__ __launch_bounds__(256) void ensemble_dw_sum_kernel(const float* __restrict__ part, long rows, int G,
                                                              float* __restrict__ dtheta) {
  __shared__ float red[G_MAX][256];
  const int t = threadIdx.x;
  float acc[G_MAX];
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) acc[g] = 0.0f;
  for (long r = t; r < rows; r += 256) {
#pragma unroll
    for (int g = 0; g < G_MAX; ++g)
      if (g < G) acc[g] += part[r * G + g];
  }
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) red[g][t] = acc[g];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int g = 0; g < G_MAX; ++g) red[g][t] += red[g][t + s];
    }
    __syncthreads();
  }
  if (t < G) dtheta[t] = red[t][0];
}

// What the four entries check alike: the tables, G, mode and the sizes
bool ens_dims_ok(const sca_decode_heads* heads, int G, int mode, int B, int T, int C) {
  return heads && G >= 1 && G <= SCA_EVAL_MAX_HEADS && (mode == 0 || mode == 1) && B >= 1 && T >= 1 && C >= 1 &&
         ((long)B * T + 3) / 4 <= 0x7fffffffL;
}

}  // namespace

extern "C" int sca_ensemble_log_probs_bwd(const sca_decode_heads* heads, int G, const sca_ensemble_weights* weights,
                                          int mode, int B, int T, int C, const float* out, const float* dout,
                                          const sca_ensemble_grads* dlogits, void* stream) {
  const long rows = (long)B * T;
  bool ok = heads && weights && out && dout && dlogits && out != dout && G >= 1 && G <= SCA_EVAL_MAX_HEADS &&
            (mode == 0 || mode == 1) && B >= 1 && T >= 1 && C >= 1 && (rows + 3) / 4 <= 0x7fffffffL;
  double sum = 0.0;
  bool any = false;
  for (int g = 0; ok && g < G; ++g) {
    const float w = weights->w[g];
    ok = heads->logits[g] != nullptr && w > 0.0f && w <= 3.0e38f;  // NaN fails w > 0
    sum += w;
    const float* dx = dlogits->dlogits[g];
    if (!dx) continue;
    any = true;
    ok = ok && dx != out && dx != dout;
    for (int k = 0; ok && k < G; ++k)
      ok = dx != heads->logits[k] && (k == g || dx != dlogits->dlogits[k]);
  }
  if (!ok) {
    sca_set_error("sca_ensemble_log_probs_bwd: bad arguments (1 <= G <= 8 non-null tensors, G finite positive "
                  "weights, mode 0 or 1, B, T, C >= 1, out and dout non-null and distinct, every non-null gradient "
                  "tensor distinct from out, dout, the members and the other gradient tensors)");
    return SCA_ERR_ARG;
  }
  if (!any) return SCA_OK;  // no member takes a gradient: nothing to launch
  const EnsHeads h = ens_heads_of(heads, G, weights, sum);
  EnsGrads d;
  for (int g = 0; g < G_MAX; ++g) d.dx[g] = g < G ? dlogits->dlogits[g] : nullptr;
  hipLaunchKernelGGL(ensemble_log_probs_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h, d, G, mode, out, dout, rows, C);
  return sca_launch_status("sca_ensemble_log_probs_bwd");
}

extern "C" int sca_ensemble_log_probs(const sca_decode_heads* heads, int G, const sca_ensemble_weights* weights,
                                      int mode, int B, int T, int C, float* out, void* stream) {
  const long rows = (long)B * T;
  bool ok = heads && weights && out && G >= 1 && G <= SCA_EVAL_MAX_HEADS && (mode == 0 || mode == 1) && B >= 1 &&
            T >= 1 && C >= 1 && (rows + 3) / 4 <= 0x7fffffffL;
  double sum = 0.0;
  for (int g = 0; ok && g < G; ++g) {
    const float w = weights->w[g];
    ok = heads->logits[g] != nullptr && heads->logits[g] != out && w > 0.0f && w <= 3.0e38f;  // NaN fails w > 0
    sum += w;
  }
  if (!ok) {
    sca_set_error("sca_ensemble_log_probs: bad arguments (1 <= G <= 8 non-null tensors other than out, G finite "
                  "positive weights, mode 0 or 1, B, T, C >= 1)");
    return SCA_ERR_ARG;
  }
  const EnsHeads h = ens_heads_of(heads, G, weights, sum);
  hipLaunchKernelGGL(ensemble_log_probs_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h, G, mode, out, rows, C);
  return sca_launch_status("sca_ensemble_log_probs");
}

// ---- learned weights: W = softmax(weight_logits), read from the device -------------------------
extern "C" int sca_ensemble_log_probs_dw(const sca_decode_heads* heads, int G, const float* weight_logits, int mode,
                                         int B, int T, int C, float* out, void* stream) {
  bool ok = ens_dims_ok(heads, G, mode, B, T, C) && weight_logits && out && weight_logits != out;
  for (int g = 0; ok && g < G; ++g)
    ok = heads->logits[g] != nullptr && heads->logits[g] != out && heads->logits[g] != weight_logits;
  if (!ok) {
    sca_set_error("sca_ensemble_log_probs_dw: bad arguments (1 <= G <= 8 non-null tensors other than out and "
                  "weight_logits, weight_logits and out non-null and distinct, mode 0 or 1, B, T, C >= 1)");
    return SCA_ERR_ARG;
  }
  const long rows = (long)B * T;
  hipLaunchKernelGGL(ensemble_log_probs_dw_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), ctc_heads_of(heads, G), weight_logits, G, mode, out, rows, C);
  return sca_launch_status("sca_ensemble_log_probs_dw");
}

extern "C" long sca_ensemble_log_probs_dw_workspace_bytes(int G, int B, int T) {
  if (G < 2 || G > SCA_EVAL_MAX_HEADS || B < 1 || T < 1) return 0;  // G = 1: d theta = 0, no partials
  return 4 * (long)G * B * T;
}

extern "C" int sca_ensemble_log_probs_dw_bwd(const sca_decode_heads* heads, int G, const float* weight_logits, int mode,
                                             int B, int T, int C, const float* out, const float* dout,
                                             const sca_ensemble_grads* dlogits, float* dweight_logits, void* ws,
                                             void* stream) {
  const bool partials = dweight_logits && G >= 2;  // what needs ws
  bool ok = ens_dims_ok(heads, G, mode, B, T, C) && weight_logits && out && dout && dlogits && out != dout &&
            weight_logits != out && weight_logits != dout && (!partials || ws);
  // the tensors that are written (gradients, d theta, ws) are distinct from every other tensor
  const void* written[G_MAX + 2];
  int n = 0;
  for (int g = 0; ok && g < G; ++g) {
    ok = heads->logits[g] != nullptr && heads->logits[g] != weight_logits;
    if (dlogits->dlogits[g]) written[n++] = dlogits->dlogits[g];
  }
  const bool any = n > 0;
  if (ok && dweight_logits) written[n++] = dweight_logits;
  if (ok && partials) written[n++] = ws;
  for (int i = 0; ok && i < n; ++i) {
    const void* p = written[i];
    ok = p != out && p != dout && p != weight_logits;
    for (int k = 0; ok && k < G; ++k) ok = p != heads->logits[k];
    for (int k = 0; ok && k < i; ++k) ok = p != written[k];
  }
  if (!ok) {
    sca_set_error("sca_ensemble_log_probs_dw_bwd: bad arguments (1 <= G <= 8 non-null tensors, weight_logits, out "
                  "and dout non-null and distinct, mode 0 or 1, B, T, C >= 1, ws non-null when dweight_logits is "
                  "asked for with G >= 2, every non-null gradient tensor, dweight_logits and ws distinct from out, "
                  "dout, weight_logits, the members and each other)");
    return SCA_ERR_ARG;
  }
  if (!any && !dweight_logits) return SCA_OK;  // nothing takes a gradient: nothing to launch
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dweight_logits && !partials) {  // G = 1: W = 1 whatever theta is
    if (hipMemsetAsync(dweight_logits, 0, sizeof(float), st) != hipSuccess) {
      (void)hipGetLastError();
      sca_set_error("sca_ensemble_log_probs_dw_bwd: clearing dweight_logits failed");
      return SCA_ERR_LAUNCH;
    }
    if (!any) return SCA_OK;
  }
  const long rows = (long)B * T;
  EnsGrads d;
  for (int g = 0; g < G_MAX; ++g) d.dx[g] = g < G ? dlogits->dlogits[g] : nullptr;
  float* part = partials ? static_cast<float*>(ws) : nullptr;
  hipLaunchKernelGGL(ensemble_log_probs_dw_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                     ctc_heads_of(heads, G), d, weight_logits, G, mode, out, dout, part, rows, C);
  if (partials)
    hipLaunchKernelGGL(ensemble_dw_sum_kernel, dim3(1), dim3(256), 0, st, part, rows, G, dweight_logits);
  return sca_launch_status("sca_ensemble_log_probs_dw_bwd");
}
