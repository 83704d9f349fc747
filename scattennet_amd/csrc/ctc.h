// What the recognition-head files share: the CTC arithmetic of heads.hip (CTC loss), decode.hip
// (decoders), align.hip (forced alignment), ensemble.hip (head ensemble) and mwer.hip (MWER
// loss), which must agree bitwise, the row-statistics pass and the by-value head table.
//
// The three lattice recursions are NOT here, on purpose: the CTC loss's 256-thread alpha / beta
// kernel (S <= 1023, one workgroup per clip), MWER's wave-private recursion (H <= 128, one wave
// per hypothesis) and the aligner's banded Viterbi (max with back-pointers instead of a sum)
// parallelise differently.  Merging them would change kernels, not share code.
#pragma once
#include "common.h"

constexpr float NEG_INF = -__builtin_huge_valf();

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// log-sum-exp of a lattice cell's three predecessors; all -inf stays -inf
__device__ __forceinline__ float lse3(float a, float b, float c) {
  float m = fmaxf(a, fmaxf(b, c));
  if (m == NEG_INF) m = 0.0f;
  return __logf(__expf(a - m) + __expf(b - m) + __expf(c - m)) + m;
}

// log_softmax(x) from the row statistics, with torch's (x - max) - log(sum) order, and the
// log_probs element of the CTC loss, clamp(log_softmax(x), -100, 0)
__device__ __forceinline__ float ctc_lp_raw(float x, float m, float ls) { return (x - m) - ls; }
__device__ __forceinline__ float ctc_lp(float raw) { return fminf(fmaxf(raw, -100.0f), 0.0f); }

// log(exp(l1) + exp(l2)) of the two end states of the last frame; -inf: the labels do not fit
__device__ __forceinline__ float ctc_end_loglik(float l1, float l2) {
  float m = fmaxf(l1, l2);
  if (m == NEG_INF) m = 0.0f;
  return __logf(__expf(l1 - m) + __expf(l2 - m)) + m;
}

// One wave over one row xr of C logits: lane 0 writes stat[0] = max and stat[1] =
// log(sum exp(x - max)).  One body under both row passes below, so they agree bitwise.
__device__ __forceinline__ void ctc_row_stat(const float* xr, int C, int lane, float* stat) {
  float m = NEG_INF;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  float s = 0.0f;
  for (int c = lane; c < C; c += 64) s += __expf(xr[c] - m);
  s = wave_sum(s);
  if (lane == 0) {
    stat[0] = m;
    stat[1] = __logf(s);
  }
}

// The prior of one labelling h of len tokens under the bigram gloss model (include/scatten.h,
// sca_nbest_rescore), by one wave: lm_weight * lm(h) + length_bonus * len.  lm: NULL (lm(h) = 0)
// or the dense (C, C) table; class 0 on either side is the sentence boundary, so lm(empty) =
// lm[0, 0].  The lanes stride over the len + 1 independent gathers, a butterfly sums them in a
// fixed order; every lane returns the value.  One body under the rescorer and the MWER loss.
__device__ __forceinline__ float ctc_bigram_prior(const float* __restrict__ lm, int C, const int* __restrict__ h,
                                                  int len, int lane, float lm_weight, float length_bonus) {
  float acc = 0.0f;
  if (lm) {
    for (int i = lane; i <= len; i += 64) {
      const int p = i == 0 ? 0 : clampi(h[i - 1], 0, C - 1), c = i == len ? 0 : clampi(h[i], 0, C - 1);
      acc += lm[(long)p * C + c];
    }
    acc = wave_sum(acc);
  }
  return lm_weight * acc + length_bonus * (float)len;
}

// The backoff n-gram gloss model (include/scatten.h, sca_ngram_lm) by value in the kernel
// arguments: a sorted trie, bigram rows by context in CSR form, trigram rows by bigram entry.
// order = 0 stands for "no model" (the entry points' lm = NULL).
using NgramLm = sca_ngram_lm;

// The entry of tok in the ascending row [lo, hi) of toks (n entries in all), or -1.  The range is
// clamped into [0, n] first and shrinks in every step: a corrupt row pointer can neither read
// out of bounds nor loop.
__device__ __forceinline__ int ngram_find(const int* __restrict__ toks, int lo, int hi, int n, int tok) {
  int a = clampi(lo, 0, n), b = clampi(hi, a, n);
  const int end = b;
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (toks[mid] < tok) {
      a = mid + 1;
    } else {
      b = mid;
    }
  }
  return a < end && toks[a] == tok ? a : -1;
}

// p2(w | v): the stored bigram, or uni_bo[v] + uni_lp[w]
__device__ __forceinline__ float ngram_p2(const NgramLm& m, int v, int w) {
  const int j = ngram_find(m.bi_tok, m.bi_ptr[v], m.bi_ptr[v + 1], m.n_bi, w);
  return j >= 0 ? m.bi_lp[j] : m.uni_bo[v] + m.uni_lp[w];
}

// p3(w | u, v): the stored trigram; else bi_bo[u, v] + p2(w | v) with (u, v) stored; else p2(w | v)
__device__ __forceinline__ float ngram_p3(const NgramLm& m, int u, int v, int w) {
  const int c = ngram_find(m.bi_tok, m.bi_ptr[u], m.bi_ptr[u + 1], m.n_bi, v);
  if (c < 0) return ngram_p2(m, v, w);
  const int t = ngram_find(m.tri_tok, m.tri_ptr[c], m.tri_ptr[c + 1], m.n_tri, w);
  return t >= 0 ? m.tri_lp[t] : m.bi_bo[c] + ngram_p2(m, v, w);
}

// ctc_bigram_prior's contract for the backoff n-gram model of order 1 to 3: path = [0] + h + [0],
// lm(h) = sum_{k = 1 .. len + 1} p(path[k] | the order - 1 elements before it), the term at k = 1
// with one element of context at most.  The lanes stride over the len + 1 independent look-ups
// (up to three binary searches each, plain loads), the same butterfly sums them; every lane
// returns lm_weight * lm(h) + length_bonus * len.  Tokens are clamped into [0, C) only to stay in
// bounds.
__device__ __forceinline__ float ctc_ngram_prior(const NgramLm& m, const int* __restrict__ h, int len, int lane,
                                                 float lm_weight, float length_bonus) {
  float acc = 0.0f;
  if (m.order >= 1) {
    for (int i = lane; i <= len; i += 64) {
      const int w = i == len ? 0 : clampi(h[i], 0, m.C - 1);
      float term;
      if (m.order == 1) {
        term = m.uni_lp[w];
      } else {
        const int v = i == 0 ? 0 : clampi(h[i - 1], 0, m.C - 1);
        if (m.order == 2 || i == 0) {
          term = ngram_p2(m, v, w);
        } else {
          term = ngram_p3(m, i == 1 ? 0 : clampi(h[i - 2], 0, m.C - 1), v, w);
        }
      }
      acc += term;
    }
    acc = wave_sum(acc);
  }
  return lm_weight * acc + length_bonus * (float)len;
}

// The prior of a kernel as a functor: the dense table (lm = NULL: lm(h) = 0) or the trie
struct CtcBigramPrior {
  const float* lm;
  int C;
  __device__ __forceinline__ float operator()(const int* __restrict__ h, int len, int lane, float lm_weight,
                                              float length_bonus) const {
    return ctc_bigram_prior(lm, C, h, len, lane, lm_weight, length_bonus);
  }
};

struct CtcNgramPrior {
  NgramLm m;
  __device__ __forceinline__ float operator()(const int* __restrict__ h, int len, int lane, float lm_weight,
                                              float length_bonus) const {
    return ctc_ngram_prior(m, h, len, lane, lm_weight, length_bonus);
  }
};

// The validation of an entry point's `lm` (NULL allowed): order in 1..3, 1 <= C <= SCA_CTC_MAX_C,
// counts >= 0 and the arrays of the orders in use; the by-value copy, order 0 for NULL.
inline bool ctc_ngram_ok(const sca_ngram_lm* lm) {
  if (!lm) return true;
  bool ok = lm->order >= 1 && lm->order <= 3 && lm->C >= 1 && lm->C <= SCA_CTC_MAX_C && lm->n_bi >= 0 &&
            lm->n_tri >= 0 && lm->uni_lp;
  if (ok && lm->order >= 2) ok = lm->uni_bo && lm->bi_ptr && (lm->n_bi == 0 || (lm->bi_tok && lm->bi_lp));
  if (ok && lm->order >= 3)
    ok = lm->tri_ptr && (lm->n_bi == 0 || lm->bi_bo) && (lm->n_tri == 0 || (lm->tri_tok && lm->tri_lp));
  return ok;
}

inline NgramLm ctc_ngram_of(const sca_ngram_lm* lm) { return lm ? *lm : NgramLm{}; }

// heads.hip: ctc_row_stat over the rows of one tensor, rowstat (rows, 2); the CTC loss, the MWER
// loss and a decoder call over one tensor use it
__attribute__((visibility("hidden"))) void sca_ctc_rowstat_launch(const float* x, float* rowstat, long rows, int C,
                                                                  hipStream_t st);
// decode.hip: the same over every (g, b, t) row of G heads, rowstat (G, rows_per_head, 2); the
// grouped decoders (G > 1) and the aligner use it.  The caller validates heads and G.
__attribute__((visibility("hidden"))) void sca_ctc_rowstat_heads_launch(const sca_decode_heads* heads, int G,
                                                                        float* rowstat, long rows_per_head, int C,
                                                                        hipStream_t st);

// The logit tensors of the G heads one launch works on, by value in the kernel arguments.  A
// (head, clip) pair is "clip" n = g B + b of the workspaces and the outputs, so a single-head
// entry point is the case G = 1.  The slots past G repeat head 0.
struct CtcHeads {
  const float* x[SCA_EVAL_MAX_HEADS];
};

// head g's tensor: a uniform select chain, so the by-value table stays in scalar registers
__device__ __forceinline__ const float* ctc_head(const CtcHeads& h, int g) {
  const float* p = h.x[0];
#pragma unroll
  for (int i = 1; i < SCA_EVAL_MAX_HEADS; ++i) p = g == i ? h.x[i] : p;
  return p;
}

inline CtcHeads ctc_heads_of(const sca_decode_heads* heads, int G) {
  CtcHeads h = {};
  for (int g = 0; g < SCA_EVAL_MAX_HEADS; ++g) h.x[g] = heads->logits[g < G ? g : 0];
  return h;
}

// The tail of a gradient row of a loss over log_probs = clamp(log_softmax(x), -100, 0), by a
// workgroup of NT threads: g[c] = g_of(c, raw) is d loss / d log_probs[c], the clamp's backward
// closes it where raw = log_softmax(x)[c] is outside [-100, 0], and the log-softmax backward is
// dx[c] = g[c] - softmax(x)[c] sum g, the sum over the waves in index order.  g_s holds C floats
// of LDS (g_of may read its own cell), red one per wave.
template <int NT, class GradOf>
__device__ __forceinline__ void ctc_grad_row_tail(const float* __restrict__ xr, float* __restrict__ dr, int C, float m,
                                                  float ls, float* g_s, float* red, int tid, GradOf g_of) {
  float part = 0.0f;
  for (int c = tid; c < C; c += NT) {
    const float raw = ctc_lp_raw(xr[c], m, ls);
    float g = g_of(c, raw);
    if (!(raw >= -100.0f && raw <= 0.0f)) g = 0.0f;  // clamp(-100, 0) backward
    g_s[c] = g;
    part += g;
  }
  part = wave_sum(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  float G = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) G += red[w];
  for (int c = tid; c < C; c += NT) dr[c] = g_s[c] - __expf(ctc_lp_raw(xr[c], m, ls)) * G;
}
