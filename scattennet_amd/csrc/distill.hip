// Ensemble distillation (include/scatten.h, sca_distill_heads_fwd / _bwd): SeqKD
// of S students against the ensemble of G members, the teacher formed on the fly and never stored.
// By definition losses[s] = sca_seqkd_fwd(student_s, sca_ensemble_log_probs(members, W, mode), ...);
// as a composition that is 1 + 3 S launches and a (B, T, C) teacher written and read back.  Here
// the forward is two launches (the rows, then one finalize for all S) and the backward one,
// whatever G and S are.
//
// One wave per (row, student) pair, four rows per 256-thread workgroup, grid.y = the student: every
// wave forms the teacher of its row itself, so S students put S times the waves in flight (at
// B T = 512 rows one student alone fills half the CUs).  Per row only q = softmax(e[start:] / temp)
// of the ensemble e matters, so
//   * mode 1 takes u = sum_g W_g lp_g as e: the normalisation of u cancels in the softmax;
//   * G = 1 takes the member's logits as e: its log-sum-exp cancels too.  That case runs the row
//     arithmetic of seqkd.h, the one under sca_seqkd_*, and is bitwise that call per student.
// For G >= 2 the members' row statistics are member_stat's (ensemble.h) and a lane owns the
// elements [V (l + 64 k), V (l + 64 k) + V) of every pass: V = 4 (16-byte loads) where every row
// involved starts on a 16-byte boundary and C % 4 == 0, V = 1 otherwise.  The columns < start are
// masked per element: with start = 1 the first pack of a vector row straddles the excluded column.
// No atomics, no LDS outside the finalize; every sum runs in a fixed order and a row's result
// depends on nothing but the row, so a replayed capture is bitwise the eager call.
//
// ws (floats), R = B T: S blocks of sca_seqkd's layout, row_loss[R] | stats[4R] | dscale[1], then
// for G >= 2 the members' statistics (S, R, G, 2) — per student, so no two waves share a cell.
#include "ensemble.h"
#include "seqkd.h"

namespace {

constexpr int S_MAX = SCA_DISTILL_MAX_STUDENTS;

// The students of one launch, by value in the kernel arguments: entry j of the grid's y axis.
// slot: the student's index in losses, dlosses and ws (the backward lists only the students that
// take a gradient).
struct DistStudents {
  const float* s[S_MAX];
  float* ds[S_MAX];
  float weight_t2[S_MAX];
  int slot[S_MAX];
};

struct DistArgs {
  EnsHeads h;          // the members; w / lw from the host, or filled from theta by every wave
  const float* theta;  // null: host weights
  int G, mode, S;
  int R, C, start;
  float inv_temp, lo, hi;
  int T;  // valid != null: rows are (b, t), t = row % T, and only t < nv take part
  const int* valid;
  int shift;
};

// entry i of a by-value table: a uniform select chain, so the table stays in scalar registers
template <class V, int N>
__device__ __forceinline__ V pick(const V (&a)[N], int i) {
  V v = a[0];
#pragma unroll
  for (int k = 1; k < N; ++k) v = i == k ? a[k] : v;
  return v;
}

__device__ __forceinline__ KdArgs kd_args_of(const DistArgs& a, const float* s, float weight_t2) {
  return KdArgs{s, a.h.x.x[0], a.R, a.C, a.start, a.inv_temp, weight_t2, a.lo, a.hi, a.T, a.valid, a.shift};
}

__device__ __forceinline__ long kd_block(const DistArgs& a) { return 5L * a.R + 1; }

__device__ __forceinline__ bool row_padded(const DistArgs& a, long row) {
  return a.valid && (int)(row % a.T) >= valid_len(a.valid, a.shift, a.T);
}

// One pack of the teacher's row e, with ensemble_row's arithmetic on the members' statistics:
//   mode 0: e[c] = M + log sum_g exp(a_g - M), a_g = lp_g[c] + log W_g, M = max_g a_g;
//   mode 1: e[c] = sum_g W_g lp_g[c] (g ascending), not normalised.
template <int V>
__device__ __forceinline__ Pack<V> teacher_pack(const EnsHeads& h, int G, int mode, long off, int c,
                                                const float (&m)[G_MAX], const float (&ls)[G_MAX]) {
  Pack<V> o;
  if (mode == 0) {
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
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int g = 0; g < G_MAX; ++g)
        if (g < G) s += __expf(a[g][i] - M[i]);
      o.v[i] = M[i] + __logf(s);
    }
    return o;
  }
#pragma unroll
  for (int i = 0; i < V; ++i) o.v[i] = 0.0f;
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    if (g < G) {
      const Pack<V> x = ldv<V>(h.x.x[g] + off + c);
#pragma unroll
      for (int i = 0; i < V; ++i) o.v[i] = fmaf(h.w[g], ctc_lp_raw(x.v[i], m[g], ls[g]), o.v[i]);
    }
  }
  return o;
}

// One (row, student) by one wave, G >= 2.  sr: the student's row; wss: the student's block of ws;
// mst: the (G, 2) cells of the members' statistics of this (student, row).
template <int V>
__device__ __forceinline__ void distill_row(const EnsHeads& h, const DistArgs& a, const float* __restrict__ sr,
                                            long off, float* __restrict__ wss, float* __restrict__ mst, long row,
                                            int lane) {
  const int G = a.G, C = a.C, start = a.start;
  const float it = a.inv_temp;
  float m[G_MAX], ls[G_MAX];
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    m[g] = 0.0f;
    ls[g] = 0.0f;
    if (g < G) member_stat<V>(h.x.x[g] + off, C, lane, m[g], ls[g]);
  }
  float ms = NEG_INF, mq = NEG_INF;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> e = teacher_pack<V>(h, G, a.mode, off, c, m, ls), x = ldv<V>(sr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (c + i >= start) {
        ms = fmaxf(ms, x.v[i] * it);
        mq = fmaxf(mq, e.v[i] * it);
      }
    }
  }
  ms = wave_max(ms);
  mq = wave_max(mq);
  float ss = 0.0f, sq = 0.0f;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> e = teacher_pack<V>(h, G, a.mode, off, c, m, ls), x = ldv<V>(sr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (c + i >= start) {
        ss += __expf(x.v[i] * it - ms);
        sq += __expf(e.v[i] * it - mq);
      }
    }
  }
  const float lss = __logf(wave_sum(ss));
  const float lsq = __logf(wave_sum(sq));
  // KLDivLoss (log_target=False): p (log p - log_softmax(student)), 0 where p underflows
  float acc = 0.0f;
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> e = teacher_pack<V>(h, G, a.mode, off, c, m, ls), x = ldv<V>(sr + c);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (c + i >= start) {
        const float lp = (e.v[i] * it - mq) - lsq;
        const float lsm = (x.v[i] * it - ms) - lss;
        const float p = __expf(lp);
        acc += p > 0.0f ? p * (lp - lsm) : 0.0f;
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    wss[row] = acc;
    float* st = wss + a.R + 4 * row;
    st[0] = ms; st[1] = lss; st[2] = mq; st[3] = lsq;
  }
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {  // one predicated store per member: m[lane] would index the array
    if (g < G && lane == g) {
      mst[2 * g] = m[g];
      mst[2 * g + 1] = ls[g];
    }
  }
}

// The gradient row of one (row, student), G >= 2: the teacher recomputed from the members with the
// saved statistics; zeros in the columns < start.
template <int V>
__device__ __forceinline__ void distill_grad_row(const EnsHeads& h, const DistArgs& a, const float* __restrict__ sr,
                                                 float* __restrict__ dr, long off, const float* __restrict__ wss,
                                                 const float* __restrict__ mst, float k, long row, int lane) {
  const int G = a.G, C = a.C, start = a.start;
  const float it = a.inv_temp;
  float m[G_MAX], ls[G_MAX];
#pragma unroll
  for (int g = 0; g < G_MAX; ++g) {
    m[g] = g < G ? mst[2 * g] : 0.0f;
    ls[g] = g < G ? mst[2 * g + 1] : 0.0f;
  }
  const float* st = wss + a.R + 4 * row;
  const float ms = st[0], lss = st[1], mq = st[2], lsq = st[3];
  for (int c = lane * V; c < C; c += 64 * V) {
    const Pack<V> e = teacher_pack<V>(h, G, a.mode, off, c, m, ls), x = ldv<V>(sr + c);
    Pack<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float lsm = (x.v[i] * it - ms) - lss;
      const float lp = (e.v[i] * it - mq) - lsq;
      r.v[i] = c + i >= start ? k * (__expf(lsm) - __expf(lp)) : 0.0f;
    }
    stv<V>(dr + c, r);
  }
}

// grid (ceil(R / 4), S): the row losses and statistics of every (row, student)
__global__ __launch_bounds__(256) void distill_rows_kernel(DistArgs a, DistStudents st, float* ws) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.R) return;  // no barrier below: a wave without a row leaves
  const int j = blockIdx.y;
  const float* s = pick(st.s, j);
  float* wss = ws + j * kd_block(a);
  if (a.G == 1) {  // the member's logits are the teacher's: sca_seqkd's own row
    const KdArgs k = kd_args_of(a, s, 0.0f);
    if (a.valid)
      kd_row<true>(k, wss, row, lane);
    else
      kd_row<false>(k, wss, row, lane);
    return;
  }
  if (row_padded(a, row)) {  // the members' statistics of a padded row are never read
    if (lane == 0) {
      wss[row] = 0.0f;
      float* z = wss + a.R + 4 * row;
      z[0] = 0.0f; z[1] = 0.0f; z[2] = 0.0f; z[3] = 0.0f;
    }
    return;
  }
  EnsHeads h = a.h;
  if (a.theta) ens_device_weights(a.theta, a.G, h.w, h.lw);
  const long off = row * a.C;
  float* mst = ws + a.S * kd_block(a) + ((long)j * a.R + row) * 2 * a.G;
  uintptr_t bits = reinterpret_cast<uintptr_t>(s + off) | (uintptr_t)(a.C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < a.G) bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
  if ((bits & 15) == 0)
    distill_row<4>(h, a, s + off, off, wss, mst, row, lane);
  else
    distill_row<1>(h, a, s + off, off, wss, mst, row, lane);
}

// grid (S): workgroup j sums student j's row losses in sca_seqkd's fixed order
__global__ __launch_bounds__(256) void distill_finalize_kernel(DistArgs a, DistStudents st, float* ws, float* losses) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const KdArgs k = kd_args_of(a, nullptr, pick(st.weight_t2, j));
  float* wss = ws + j * kd_block(a);
  if (a.valid)
    kd_finalize<true>(k, wss, losses + j, red, threadIdx.x);
  else
    kd_finalize<false>(k, wss, losses + j, red, threadIdx.x);
}

// grid (ceil(R / 4), n): the gradient rows of the n students that take one
__global__ __launch_bounds__(256) void distill_grad_kernel(DistArgs a, DistStudents st, const float* ws,
                                                           const float* dlosses) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.R) return;  // no barrier below: a wave without a row leaves
  const int j = blockIdx.y;
  const float* s = pick(st.s, j);
  float* ds = pick(st.ds, j);
  const int slot = pick(st.slot, j);
  const float* wss = ws + slot * kd_block(a);
  if (a.G == 1) {
    const KdArgs k = kd_args_of(a, s, 0.0f);
    if (a.valid)
      kd_grad_row<true>(k, wss, dlosses + slot, ds, nullptr, row, lane);
    else
      kd_grad_row<false>(k, wss, dlosses + slot, ds, nullptr, row, lane);
    return;
  }
  const long off = row * a.C;
  if (row_padded(a, row)) {  // exact zeros behind the valid frames
    for (int c = lane; c < a.C; c += 64) ds[off + c] = 0.0f;
    return;
  }
  EnsHeads h = a.h;
  if (a.theta) ens_device_weights(a.theta, a.G, h.w, h.lw);
  const float k = dlosses[slot] * wss[5L * a.R] * a.inv_temp;
  const float* mst = ws + a.S * kd_block(a) + ((long)slot * a.R + row) * 2 * a.G;
  uintptr_t bits =
      reinterpret_cast<uintptr_t>(s + off) | reinterpret_cast<uintptr_t>(ds + off) | (uintptr_t)(a.C & 3);
#pragma unroll
  for (int g = 0; g < G_MAX; ++g)
    if (g < a.G) bits |= reinterpret_cast<uintptr_t>(h.x.x[g] + off);
  if ((bits & 15) == 0)
    distill_grad_row<4>(h, a, s + off, ds + off, off, wss, mst, k, row, lane);
  else
    distill_grad_row<1>(h, a, s + off, ds + off, off, wss, mst, k, row, lane);
}

bool sizes_ok(int S, int G, int B, int T) {
  return S >= 1 && S <= S_MAX && G >= 1 && G <= SCA_EVAL_MAX_HEADS && B >= 1 && T >= 1 &&
         (long)B * T <= 0x7fffffffL;
}

// What the two entries check alike; on success `a` holds everything but the students.
bool distill_args(const sca_decode_heads* members, int G, const sca_ensemble_weights* weights,
                  const float* weight_logits, int mode, const sca_distill_students* students, int S, int B, int T,
                  int C, int start, float temp, const int* valid_frames, int shift, DistArgs& a) {
  bool ok = sizes_ok(S, G, B, T) && members && students && (mode == 0 || mode == 1) && C >= 1 && start >= 0 &&
            start < C && temp > 0.0f && (weights != nullptr) != (weight_logits != nullptr) &&
            (!valid_frames || (shift >= 0 && shift <= 30));
  double sum = 0.0;
  for (int g = 0; ok && g < G; ++g) {
    ok = members->logits[g] != nullptr && members->logits[g] != weight_logits;
    if (ok && weights) {
      const float w = weights->w[g];
      ok = w > 0.0f && w <= 3.0e38f;  // NaN fails w > 0
      sum += w;
    }
  }
  for (int s = 0; ok && s < S; ++s) ok = students->logits[s] != nullptr;
  if (!ok) return false;
  if (weights) {
    a.h = ens_heads_of(members, G, weights, sum);
  } else {
    a.h.x = ctc_heads_of(members, G);
    for (int g = 0; g < G_MAX; ++g) a.h.w[g] = a.h.lw[g] = 0.0f;
  }
  a.theta = weight_logits;
  a.G = G; a.mode = mode; a.S = S;
  a.R = B * T; a.C = C; a.start = start;
  a.inv_temp = 1.0f / temp; a.lo = 0.0f; a.hi = 0.0f;
  a.T = T; a.valid = valid_frames; a.shift = shift;
  return true;
}

// p (written by the call) is none of the call's inputs
bool not_an_input(const void* p, const sca_decode_heads* members, int G, const sca_distill_students* students, int S,
                  const float* weight_logits, const int* valid_frames) {
  bool ok = p != weight_logits && p != valid_frames;
  for (int g = 0; ok && g < G; ++g) ok = p != members->logits[g];
  for (int s = 0; ok && s < S; ++s) ok = p != students->logits[s];
  return ok;
}

int distill_bad(const char* name) {
  char msg[640];
  snprintf(msg, sizeof(msg),
           "%s: bad arguments (1 <= G <= 8 non-null members, 1 <= S <= 8 non-null students, exactly one of weights "
           "(G finite positive numbers) and weight_logits, mode 0 or 1, B, T, C >= 1, B T < 2^31, 0 <= start < C, "
           "temp > 0, 0 <= shift <= 30 with valid_frames, the outputs and ws non-null and distinct from every input "
           "and from each other)",
           name);
  sca_set_error(msg);
  return SCA_ERR_ARG;
}

}  // namespace

extern "C" long sca_distill_heads_workspace_floats(int S, int G, int B, int T) {
  if (!sizes_ok(S, G, B, T)) return 0;
  const long R = (long)B * T;
  return S * (5 * R + 1) + (G >= 2 ? 2L * S * R * G : 0);
}

extern "C" int sca_distill_heads_fwd(const sca_decode_heads* members, int G, const sca_ensemble_weights* weights,
                                     const float* weight_logits, int mode, const sca_distill_students* students, int S,
                                     int B, int T, int C, int start, float temp, float lo, float hi,
                                     const int* valid_frames, int shift, float* losses, float* ws, void* stream) {
  DistArgs a;
  bool ok = distill_args(members, G, weights, weight_logits, mode, students, S, B, T, C, start, temp, valid_frames,
                         shift, a) &&
            losses && ws && (const void*)losses != (const void*)ws &&
            not_an_input(losses, members, G, students, S, weight_logits, valid_frames) &&
            not_an_input(ws, members, G, students, S, weight_logits, valid_frames);
  if (!ok) return distill_bad("sca_distill_heads_fwd");
  a.lo = lo;
  a.hi = hi;
  DistStudents st = {};
  for (int s = 0; s < S_MAX; ++s) {
    const int k = s < S ? s : 0;
    st.s[s] = students->logits[k];
    st.weight_t2[s] = students->weight[k] * temp * temp;
    st.slot[s] = k;
  }
  hipStream_t q = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(distill_rows_kernel, dim3((unsigned)((a.R + 3L) / 4), S), dim3(256), 0, q, a, st, ws);
  hipLaunchKernelGGL(distill_finalize_kernel, dim3(S), dim3(256), 0, q, a, st, ws, losses);
  return sca_launch_status("sca_distill_heads_fwd");
}

extern "C" int sca_distill_heads_bwd(const sca_decode_heads* members, int G, const sca_ensemble_weights* weights,
                                     const float* weight_logits, int mode, const sca_distill_students* students, int S,
                                     int B, int T, int C, int start, float temp, const int* valid_frames, int shift,
                                     const float* dlosses, const float* ws, const sca_distill_grads* dstudents,
                                     void* stream) {
  DistArgs a;
  bool ok = distill_args(members, G, weights, weight_logits, mode, students, S, B, T, C, start, temp, valid_frames,
                         shift, a) &&
            dlosses && ws && dstudents;
  DistStudents st = {};
  int n = 0;
  for (int s = 0; ok && s < S; ++s) {
    float* d = dstudents->dlogits[s];
    if (!d) continue;
    ok = (const void*)d != (const void*)dlosses && (const void*)d != (const void*)ws &&
         not_an_input(d, members, G, students, S, weight_logits, valid_frames);
    for (int k = 0; ok && k < n; ++k) ok = d != st.ds[k];
    st.s[n] = students->logits[s];
    st.ds[n] = d;
    st.slot[n] = s;
    ++n;
  }
  if (!ok) return distill_bad("sca_distill_heads_bwd");
  if (n == 0) return SCA_OK;  // no student takes a gradient: nothing to launch
  for (int s = n; s < S_MAX; ++s) {
    st.s[s] = st.s[0];
    st.ds[s] = st.ds[0];
    st.slot[s] = st.slot[0];
  }
  hipLaunchKernelGGL(distill_grad_kernel, dim3((unsigned)((a.R + 3L) / 4), n), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, st, ws, dlosses);
  return sca_launch_status("sca_distill_heads_bwd");
}
