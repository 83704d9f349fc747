// Evaluation path of the reference's evaluate_fn (opt.py:50-128) on the device:
//   * CTC decoding of the recognition-head logits: best path (greedy) and prefix beam search,
//     the algorithm of tf.nn.ctc_beam_search_decoder (utils.py:164-189, top_paths = 1, no
//     label merging inside the search), in log space.  Blank = class 0: the reference's
//     column rotation and its "+ 1" cancel, so output ids are the model's class indices.
//   * WER counts (metrics.py:2793-2907): the weighted edit-distance matrix (del 3, ins 3,
//     sub 4; on equal tokens the cell IS the diagonal value, not a minimum) and the
//     back-trace in the reference's order of preference (correct, substitution, insertion,
//     deletion).  The reference keeps the matrix in uint8, which wraps once 3 (R + H) > 255;
//     here the cells are 16-bit (3 * 256 = 768 at most), so that defect is NOT reproduced.
//   * The second pass over the beam (no counterpart in the reference): the N best labellings
//     of the same search, merged after the groupby and re-sorted, their rescoring with a bigram
//     gloss model, the posterior over the list and MBR selection under the WER alignment above.
// The T frames of a clip are a dependent chain (like the alpha recursion of the CTC loss),
// so a clip is one workgroup; everything that does not depend on the beam (row normaliser,
// the W + 1 best classes of every frame) is computed beforehand by row-parallel launches.
// No float atomics; every sum runs in a fixed order: results are deterministic.
#include "ctc.h"
#include "wer_pair.h"

namespace {

constexpr int NONE = 0x7fffffff;
constexpr int DEC_MAX_W = SCA_CTC_MAX_BEAM;
constexpr int DEC_MAX_ITEMS = DEC_MAX_W * (DEC_MAX_W + 1) + DEC_MAX_W;  // candidates + updated beams
constexpr int KEY_CAND = 64;                                             // keys below: updated beams
constexpr int DEC_ARENA_LDS = 2048;                                      // arena nodes mirrored in LDS
constexpr int DEC_FUSE_LIST = 256;  // fused search: labels above the threshold that the rank count merges
constexpr int DEC_FUSE_CHUNK = 24;  // fused search: labels per lane loaded together (64 * 24 >= 1124 - 1)

struct DecDims {
  int B, T, C, W;
};

// workspace layout, N = G B clips: rowstat float[2 NT] | cls int[NT (W+1)] | clp float[NT (W+1)] |
// arena u64[N (T W + 1)] (dec_pl words).  The greedy path keeps its per-frame arg-max in cls.
struct DecWs {
  float* rowstat;
  int* cls;
  float* clp;
  unsigned long long* arena;
  __host__ __device__ DecWs(void* ws, DecDims d, int G = 1) {
    const long BT = (long)G * d.B * d.T, K = d.W + 1;
    rowstat = static_cast<float*>(ws);
    cls = reinterpret_cast<int*>(rowstat + 2 * BT);
    clp = reinterpret_cast<float*>(cls + BT * K);
    arena = reinterpret_cast<unsigned long long*>(clp + BT * K);  // 2 BT (K + 1) floats in front: 8-byte aligned
  }
};

// The bigram model of the fused search (sca_ctc_beam_decode_fused_nbest): lm (C, C) or NULL.
struct DecLm {
  const float* lm;
  float weight, bonus;
};

__device__ __forceinline__ float logaddexp(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (lo == NEG_INF) return hi;
  return hi + __logf(1.0f + __expf(lo - hi));
}

// outside the frame loop: full-precision exp and log1p
__device__ __forceinline__ float logaddexp_tail(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (lo == NEG_INF) return hi;
  return hi + log1pf(expf(lo - hi));
}

// (v, c) beats (w, d): larger value, ties to the lower index
__device__ __forceinline__ bool beats(float v, int c, float w, int d) { return v > w || (v == w && c < d); }

__device__ __forceinline__ void wave_argmax(float& v, int& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o, 64);
    const int d = __shfl_xor(c, o, 64);
    if (beats(w, d, v, c)) { v = w; c = d; }
  }
}

// (value, key) as one unsigned word that orders like "larger value first, then lower key":
// the float's bits made monotone (-0 folded into +0), the key complemented below them.
// Never 0 for a finite or infinite value, so 0 marks a dropped item.
__device__ __forceinline__ unsigned long long dec_ord(float v, int key) {
  unsigned u = __float_as_uint(v + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)(NONE - key);
}
__device__ __forceinline__ int dec_ord_key(unsigned long long o) { return NONE - (int)(unsigned)(o & 0xffffffffull); }

// What a beam of the fused search ranks a label by: lp[c] + weight * lm[last, c], one rounding,
// the same value wherever it is evaluated.  lp and the bigram term go out as they enter the
// candidate.  fuse_ord: the same from the rows (row NULL: no table), as a dec_ord word with c.
__device__ __forceinline__ float fuse_key(float xv, float lmv, float weight, float m, float ls, float& lp, float& bg) {
  lp = ctc_lp_raw(xv, m, ls);
  bg = weight * lmv;
  return __fmaf_rn(weight, lmv, lp);
}
__device__ __forceinline__ unsigned long long fuse_ord(const float* __restrict__ xr, const float* __restrict__ row,
                                                        float weight, int c, float m, float ls, float& lp, float& bg) {
  return dec_ord(fuse_key(xr[c], row ? row[c] : 0.0f, weight, m, ls, lp, bg), c);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// an arena node, and a beam's identity as "child of node par by label lab", as one word
__device__ __forceinline__ unsigned long long dec_pl(int par, int lab) {
  return ((unsigned long long)(unsigned)par << 32) | (unsigned)lab;
}
__device__ __forceinline__ int dec_par(unsigned long long v) { return (int)(v >> 32); }
__device__ __forceinline__ int dec_lab(unsigned long long v) { return (int)(v & 0xffffffffull); }

// One wave per (g, b, t) row: max and log-sum-exp of the logits row, the CTC loss's row pass
// (ctc_row_stat, ctc.h) over the rows of G tensors.  A grouped decoder's first launch.
__global__ __launch_bounds__(256) void ctc_rowstat_heads_kernel(CtcHeads hx, float* __restrict__ rowstat, long rows,
                                                                long rows_per_head, int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int g = (int)(row / rows_per_head);
  ctc_row_stat(ctc_head(hx, g) + (row - g * rows_per_head) * C, C, lane, rowstat + 2 * row);
}

// One wave per (g, b, t) row: the K = min(W + 1, C - 1) labels (c != 0) with the largest
// log-probability, in descending order, ties to the lower class.  Round k takes the best
// element strictly after round k - 1's pick in that order, so nothing is marked as taken.
__global__ __launch_bounds__(256) void ctc_topk_kernel(CtcHeads hx, int G, const int* __restrict__ in_len, DecDims d,
                                                       DecWs w) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (long)G * d.B * d.T) return;
  const int n = (int)(row / d.T), t = (int)(row - (long)n * d.T);  // n = g B + b
  const int g = n / d.B, b = n - g * d.B;
  if (t >= clampi(in_len[b], 0, d.T)) return;
  const float* xr = ctc_head(hx, g) + ((long)b * d.T + t) * d.C;
  const float m = w.rowstat[2 * row], ls = w.rowstat[2 * row + 1];
  const int K = min(d.W + 1, d.C - 1);
  float pv = 0.0f;
  int pc = -1;
  for (int k = 0; k < K; ++k) {
    float bv = NEG_INF;
    int bc = NONE;
    for (int c = 1 + lane; c < d.C; c += 64) {
      const float v = ctc_lp_raw(xr[c], m, ls);
      const bool open = k == 0 || v < pv || (v == pv && c > pc);
      if (open && v > bv) { bv = v; bc = c; }  // ascending c: the first of equal values stays
    }
    wave_argmax(bv, bc);
    if (lane == 0) {
      w.cls[row * (d.W + 1) + k] = bc == NONE ? 0 : bc;  // 0: no label left above -inf
      w.clp[row * (d.W + 1) + k] = bv;
    }
    pv = bv;
    pc = bc;
  }
}

// One workgroup (one wave) per (clip, head): grid (B, G).  Beam slot state lives in LDS,
// double-buffered; slots are kept sorted by total, so slot 0 is the best beam.  A prefix is a node (parent, label)
// of the clip's arena; a candidate whose (parent, label) pair already has a node (a pruned
// prefix that comes back) takes that node again, so a prefix has one node for good and
// "is this prefix an active beam" is a comparison of node ids.  Log-probabilities are kept
// relative to the best beam's total of the previous frame (the sum of those shifts is
// carried in a double): the selection is shift-invariant and fp32 rounding then acts on
// numbers of the size of the beam's spread, not of the whole clip's log-probability.
//
// The frame loop is a latency chain, so nothing in it waits for global memory that could have
// been asked for earlier: frame t + 1's normaliser, blank logit and best labels are loaded
// during frame t, and so are frame t + 1's logits of every label a new beam can end in (the
// active beams' labels and frame t's best labels).  The first DEC_ARENA_LDS arena nodes are
// mirrored in LDS for the look-up; the hand-offs between phases are then LDS-only barriers
// that leave those loads in flight.  The beam_width best of the M <= W (W + 2) items are
// found by counting, for each item, the items in front of it (M LDS broadcast reads per
// item, no cross-lane traffic).
//
// NBEST: the same frame loop, then the tail of sca_ctc_beam_decode_nbest instead of the walk of
// slot 0: one lane per final beam walks and collapses its own prefix into the clip's cls rows
// (the per-frame best labels are dead once the loop is over, and nbest T <= T (W + 1) ints),
// equal entries merge into the first of them, a rank count re-sorts, and the wave writes the
// (nbest, T) rows out.  tokens (nbest, T), out_len / score (nbest) and count (1) per clip.
//
// FUSED (with NBEST): shallow fusion, sca_ctc_beam_decode_fused_nbest.  Every beam carries
// g(prefix), relative to slot 0's like the totals; items are ranked by total + g and the slots
// stay sorted by that key.  The frame's shared label list is not exact under a bigram term, so
// every beam selects its own K labels by lp[c] + weight * lm[last, c] (fuse_ord) over the whole
// row: the lanes stride over the row and keep their maximum, the K-th largest of the 64 maxima
// is a threshold that at least K labels reach, and only labels of the lanes whose maximum
// reaches it can.  A second pass over the row appends those labels to an LDS list by ballot, and
// a rank count over the list's (value, class) words yields the K best in order.  A list longer than DEC_FUSE_LIST (K
// lanes full of large values) falls back to K rounds of wave arg-max, ctc_topk_kernel's method.
// Both are exact, so with weight 0 and bonus 0 the item pool, and every output, is bitwise the
// unfused instantiation's.  After the last frame a rank count orders the beams by the final key
// (the closing bigram included) and the tail takes entry n from beam p_src[n].  The unfused
// instantiations contain none of this: every fused statement is under `if constexpr`.
template <bool NBEST, bool FUSED = false>
__global__ __launch_bounds__(64) void ctc_beam_kernel(CtcHeads hx, const int* __restrict__ in_len, DecDims d,
                                                      int collapse, int nbest, int* __restrict__ tokens,
                                                      int* __restrict__ out_len, float* __restrict__ score,
                                                      int* __restrict__ count, DecWs w, DecLm f) {
  static_assert(NBEST || !FUSED, "the fused search has the n-best tail only");
  constexpr int FW = FUSED ? DEC_MAX_W : 1, FI = FUSED ? DEC_MAX_ITEMS : 1, FL = FUSED ? DEC_FUSE_LIST : 1;
  __shared__ float s_g[2][FW], it_g[FI];       // g of the beams and of the items
  __shared__ int it_cls[FI];                   // an item's label
  __shared__ float l_max[FUSED ? 64 : 1];      // the lanes' maxima
  __shared__ unsigned long long f_key[FW], l_ord[FL];  // the final keys; one beam's list
  __shared__ float l_lp[FL], l_bg[FL];
  __shared__ int pk_cls[FW + 1], p_src[FW];    // one beam's K labels; the final order
  __shared__ float pk_lp[FW + 1], pk_bg[FW + 1];
  __shared__ int s_node[2][DEC_MAX_W], s_lab[2][DEC_MAX_W], s_par[2][DEC_MAX_W];
  __shared__ float s_lb[2][DEC_MAX_W], s_ll[2][DEC_MAX_W], s_tot[2][DEC_MAX_W];
  __shared__ float s_xe[2][DEC_MAX_W];  // this frame's logit of the beam's last label
  __shared__ float u_lb[DEC_MAX_W], u_ll[DEC_MAX_W];
  __shared__ float it_val[DEC_MAX_ITEMS];
  __shared__ unsigned long long it_ord[DEC_MAX_ITEMS];
  __shared__ int f_cls[DEC_MAX_W + 1];                       // this frame's best labels ...
  __shared__ float f_clp[DEC_MAX_W + 1];                     // ... and their log-probabilities
  __shared__ float n_xc[DEC_MAX_W + 1], n_xb[DEC_MAX_W];     // the next frame's logits of those / of the beams' labels
  __shared__ int sel[DEC_MAX_W], found[DEC_MAX_W];
  __shared__ unsigned long long s_pl[2][DEC_MAX_W];  // dec_pl(s_par, s_lab)
  __shared__ unsigned long long want[DEC_MAX_W];     // the node a fresh beam looks for, else ~0
  __shared__ unsigned long long a_lds[DEC_ARENA_LDS];
  __shared__ int s_len;
  const int lane = threadIdx.x;
  const int slot = (int)blockIdx.y * d.B + (int)blockIdx.x;  // the (head, clip)'s place in workspace and outputs
  const int T = d.T, C = d.C, W = d.W, KS = W + 1, K = min(W + 1, C - 1);
  const int Tb = clampi(in_len[blockIdx.x], 0, T);
  const float* __restrict__ x = ctc_head(hx, blockIdx.y) + (long)blockIdx.x * T * C;  // the clip's (T, C) logits
  unsigned long long* arena = w.arena + (long)slot * ((long)T * W + 1);
  int nn = 1, nb = 1, cur = 0;  // arena nodes, active beams, state buffer (all wave-uniform)
  double offset = 0.0;
  // the frame's beam-independent inputs, loaded one frame ahead
  float pm = 0.0f, pls = 0.0f, px0 = 0.0f, pclp = NEG_INF;
  int pcls = 0;
  auto prefetch = [&](int t) {
    const long row = (long)slot * T + t;
    pm = w.rowstat[2 * row];
    pls = w.rowstat[2 * row + 1];
    px0 = x[(long)t * C];
    if constexpr (!FUSED) {
      if (lane < K) {
        pcls = w.cls[row * KS + lane];
        pclp = w.clp[row * KS + lane];
      }
    }
  };
  if (Tb > 0) prefetch(0);
  if (lane == 0) {
    arena[0] = dec_pl(-1, 0);  // the empty prefix
    a_lds[0] = dec_pl(-1, 0);
    s_node[0][0] = 0; s_lab[0][0] = 0; s_par[0][0] = -1; s_pl[0][0] = dec_pl(-1, 0);
    s_lb[0][0] = 0.0f; s_ll[0][0] = NEG_INF; s_tot[0][0] = 0.0f; s_xe[0][0] = 0.0f;
    if constexpr (FUSED) s_g[0][0] = 0.0f;
  }
  __syncthreads();
  for (int t = 0; t < Tb; ++t) {
    const float m = pm, ls = pls, lp0 = ctc_lp_raw(px0, pm, pls);
    const int nxt = cur ^ 1;
    if constexpr (!FUSED) {
      if (lane < K) { f_cls[lane] = pcls; f_clp[lane] = pclp; }
    }
    if (lane < W) sel[lane] = -1;
    float nxc = 0.0f, nxb = 0.0f;
    if (t + 1 < Tb) {  // wave-uniform
      const float* xn = x + (long)(t + 1) * C;
      if constexpr (!FUSED) {
        if (lane < K) nxc = xn[pcls];
      }
      if (lane < nb) nxb = xn[s_lab[cur][lane]];
      prefetch(t + 1);
    }
    lds_barrier();
    // updated beams
    if (lane < nb) {
      const int e = s_lab[cur][lane], par = s_par[cur][lane];
      const float nlb = s_tot[cur][lane] + lp0;
      float nll = NEG_INF;
      if (par >= 0) {
        const float lpe = ctc_lp_raw(s_xe[cur][lane], m, ls);
        nll = s_ll[cur][lane] + lpe;
        int pj = -1;  // the parent prefix's slot: node ids of active beams are distinct
#pragma unroll 8
        for (int j = 0; j < nb; ++j) pj = s_node[cur][j] == par ? j : pj;
        if (pj >= 0) nll = logaddexp(nll, lpe + (e == s_lab[cur][pj] ? s_lb[cur][pj] : s_tot[cur][pj]));
      }
      const float tot = logaddexp(nlb, nll);
      u_lb[lane] = nlb;
      u_ll[lane] = nll;
      it_val[lane] = tot;
      if constexpr (FUSED) it_ord[lane] = dec_ord(tot + s_g[cur][lane], lane);
      else it_ord[lane] = dec_ord(tot, lane);
    }
    const int M = nb + nb * K;
    if constexpr (FUSED) {
      // extension candidates: beam j x its own K best labels by lp + weight * lm[last(j), .]
      const float* __restrict__ xr = x + (long)t * C;
      for (int j = 0; K > 0 && j < nb; ++j) {  // wave-uniform
        const int lj = s_lab[cur][j];          // 0 for the empty prefix: the sentence boundary
        const float* __restrict__ row = f.lm ? f.lm + (long)lj * C : nullptr;
        // A chunk is DEC_FUSE_CHUNK labels per lane, loaded together (one trip to L1 / L2, not one
        // per label; past the row's end the last label again, masked below) and kept in registers;
        // a row that fits one chunk is loaded once for both passes.
        float lp, bg;
        float cv[DEC_FUSE_CHUNK], clp[DEC_FUSE_CHUNK], cbg[DEC_FUSE_CHUNK];
        auto load_chunk = [&](int c0) {
          float xv[DEC_FUSE_CHUNK], lv[DEC_FUSE_CHUNK];
#pragma unroll
          for (int u = 0; u < DEC_FUSE_CHUNK; ++u) xv[u] = xr[min(c0 + lane + 64 * u, C - 1)];
#pragma unroll
          for (int u = 0; u < DEC_FUSE_CHUNK; ++u) lv[u] = row ? row[min(c0 + lane + 64 * u, C - 1)] : 0.0f;
#pragma unroll
          for (int u = 0; u < DEC_FUSE_CHUNK; ++u) cv[u] = fuse_key(xv[u], lv[u], f.weight, m, ls, clp[u], cbg[u]);
        };
        const bool one_chunk = C - 1 <= 64 * DEC_FUSE_CHUNK;
        float top = NEG_INF;  // the lane's largest value
        for (int c0 = 1; c0 < C; c0 += 64 * DEC_FUSE_CHUNK) {  // wave-uniform
          load_chunk(c0);
#pragma unroll
          for (int u = 0; u < DEC_FUSE_CHUNK; ++u) top = (c0 + lane + 64 * u < C && cv[u] > top) ? cv[u] : top;
        }
        l_max[lane] = top;
        lds_barrier();
        // A threshold that at least K labels reach: the smallest maximum among the lanes with fewer
        // than K maxima strictly above theirs (the K largest maxima are among them).  Every label
        // of the K best reaches it too, so the list below is a superset of them; ties only add to it.
        int above = 0;
#pragma unroll 16
        for (int i = 0; i < 64; ++i) above += l_max[i] > top;
        const float tau = -wave_max(above < K ? -top : NEG_INF);
        int cnt = 0;
        for (int c0 = 1; c0 < C; c0 += 64 * DEC_FUSE_CHUNK) {  // wave-uniform
          if (!one_chunk) load_chunk(c0);
#pragma unroll
          for (int u = 0; u < DEC_FUSE_CHUNK; ++u) {
            const int c = c0 + lane + 64 * u;
            const bool in = c < C && cv[u] >= tau;
            const unsigned long long mask = __ballot(in);
            if (mask == 0ull) continue;  // wave-uniform: most strides hold no such label
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            if (in && pos < DEC_FUSE_LIST) { l_ord[pos] = dec_ord(cv[u], c); l_lp[pos] = clp[u]; l_bg[pos] = cbg[u]; }
            cnt += __popcll(mask);
          }
        }
        lds_barrier();
        if (cnt <= DEC_FUSE_LIST) {  // wave-uniform
          for (int n = lane; n < cnt; n += 64) {
            const unsigned long long mine = l_ord[n];
            int rank = 0;
#pragma unroll 4
            for (int i = 0; i < cnt; ++i) rank += l_ord[i] > mine;
            if (rank < K) { pk_cls[rank] = dec_ord_key(mine); pk_lp[rank] = l_lp[n]; pk_bg[rank] = l_bg[n]; }
          }
        } else {  // round k: the best label strictly behind round k - 1's
          unsigned long long prev = ~0ull;
          for (int k = 0; k < K; ++k) {
            unsigned long long best = 0ull;
            for (int c = 1 + lane; c < C; c += 64) {
              const unsigned long long o = fuse_ord(xr, row, f.weight, c, m, ls, lp, bg);
              best = (o < prev && o > best) ? o : best;
            }
            best = wave_max_u64(best);
            if (lane == 0) {
              const int c = clampi(dec_ord_key(best), 1, C - 1);  // best != 0: K <= C - 1 labels exist
              fuse_ord(xr, row, f.weight, c, m, ls, lp, bg);
              pk_cls[k] = c; pk_lp[k] = lp; pk_bg[k] = bg;
            }
            prev = best;
          }
        }
        lds_barrier();
        if (lane < K) {
          const int c = clampi(pk_cls[lane], 1, C - 1);  // a NaN logit cannot carry it out of the row
          float v = NEG_INF;
          const unsigned long long qc = dec_pl(s_node[cur][j], c);
          bool active = false;
#pragma unroll 4
          for (int i = 0; i < nb; ++i) active |= s_pl[cur][i] == qc;
          if (!active) v = pk_lp[lane] + (c == lj ? s_lb[cur][j] : s_tot[cur][j]);
          const float gn = s_g[cur][j] + pk_bg[lane] + f.bonus;
          const int n = nb + j * K + lane;
          it_val[n] = v;
          it_g[n] = gn;
          it_cls[n] = c;
          it_ord[n] = v == NEG_INF ? 0ull : dec_ord(v + gn, KEY_CAND + j * SCA_CTC_MAX_C + c);  // -inf: dropped
        }
        lds_barrier();
      }
    }
    // extension candidates: beam j x the frame's k-th best label
    for (int n = lane; !FUSED && n < nb * K; n += 64) {
      const int j = n / K, k = n - j * K;
      const int c = f_cls[k];
      float v = NEG_INF;
      if (c > 0) {
        const unsigned long long qc = dec_pl(s_node[cur][j], c);
        bool active = false;
#pragma unroll 4
        for (int i = 0; i < nb; ++i) active |= s_pl[cur][i] == qc;
        if (!active) v = f_clp[k] + (c == s_lab[cur][j] ? s_lb[cur][j] : s_tot[cur][j]);
      }
      it_val[nb + n] = v;
      it_ord[nb + n] = v == NEG_INF ? 0ull : dec_ord(v, KEY_CAND + j * SCA_CTC_MAX_C + c);  // -inf: dropped
    }
    lds_barrier();
    // the W best by (total, key): updated beams first, then lower slot, then lower class.
    // An item's rank is the number of items in front of it; the keys are distinct.
    for (int n = lane; n < M; n += 64) {
      const unsigned long long mine = it_ord[n];
      if (mine == 0ull) continue;
      int rank = 0;
#pragma unroll 8
      for (int i = 0; i < M; ++i) rank += it_ord[i] > mine;
      if (rank < W) sel[rank] = n;
    }
    if constexpr (!FUSED) {
      if (lane < K) n_xc[lane] = nxc;
    }
    if (lane < nb) n_xb[lane] = nxb;
    lds_barrier();
    const int R = __popcll(__ballot(lane < W && sel[lane < W ? lane : 0] >= 0));
    // the new beam set, in selection order
    int node = -1, lab = 0, par = -1;
    float lb = NEG_INF, ll = NEG_INF, tot = NEG_INF, xe = 0.0f;
    [[maybe_unused]] float g = 0.0f;
    bool fresh = false;
    if (lane < R) {
      const int idx = max(sel[lane], 0);  // ranks are a permutation unless a total is NaN: stay in bounds
      tot = it_val[idx];
      if (idx < nb) {
        node = s_node[cur][idx]; lab = s_lab[cur][idx]; par = s_par[cur][idx];
        lb = u_lb[idx]; ll = u_ll[idx];
        xe = n_xb[idx];
        if constexpr (FUSED) g = s_g[cur][idx];
      } else {
        const int n = idx - nb, j = n / K, k = n - j * K;
        par = s_node[cur][j];
        if constexpr (FUSED) {  // the label is the beam's own pick: its next logit could not be asked for earlier
          lab = it_cls[idx];
          g = it_g[idx];
          if (t + 1 < Tb) xe = x[(long)(t + 1) * C + lab];
        } else {
          lab = f_cls[k];
          xe = n_xc[k];
        }
        ll = tot;
        fresh = true;
      }
      s_par[nxt][lane] = par;
      s_lab[nxt][lane] = lab;
      s_pl[nxt][lane] = dec_pl(par, lab);
      want[lane] = fresh ? dec_pl(par, lab) : ~0ull;
      found[lane] = -1;
    }
    const unsigned long long any_fresh = __ballot(fresh);
    lds_barrier();
    if (any_fresh) {  // a prefix that was pruned and comes back keeps its node
      const int nl = min(nn, DEC_ARENA_LDS);
      for (int n0 = lane; n0 < nl; n0 += 256) {  // four nodes per lane and pass: fewer dependent LDS trips
        unsigned long long nd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nd[u] = n0 + 64 * u < nl ? a_lds[n0 + 64 * u] : ~0ull;
#pragma unroll 8
        for (int r = 0; r < R; ++r) {
          const unsigned long long wr = want[r];
          if (wr == ~0ull) continue;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (wr == nd[u]) found[r] = n0 + 64 * u;
        }
      }
      for (int n = DEC_ARENA_LDS + lane; n < nn; n += 64) {  // nodes beyond the mirror
        const unsigned long long nd = arena[n];
#pragma unroll 4
        for (int r = 0; r < R; ++r)
          if (want[r] == nd) found[r] = n;
      }
    }
    lds_barrier();
    const bool alloc = fresh && found[lane < R ? lane : 0] < 0;
    const unsigned long long am = __ballot(alloc);
    if (fresh) {
      node = found[lane];
      if (alloc) {
        node = nn + __popcll(am & ((1ull << lane) - 1ull));  // < nn + W <= T W + 1
        arena[node] = dec_pl(par, lab);
        if (node < DEC_ARENA_LDS) a_lds[node] = dec_pl(par, lab);
      }
    }
    nn += __popcll(am);
    const float shift = __shfl(tot, 0, 64);  // slot 0: the best total
    if (shift != NEG_INF) {
      offset += (double)shift;
      lb -= shift; ll -= shift; tot -= shift;
    }
    if constexpr (FUSED) g -= __shfl(g, 0, 64);  // only differences of g are ever compared
    if (lane < R) {
      s_node[nxt][lane] = node;
      s_lb[nxt][lane] = lb; s_ll[nxt][lane] = ll; s_tot[nxt][lane] = tot; s_xe[nxt][lane] = xe;
      if constexpr (FUSED) s_g[nxt][lane] = g;
    }
    nb = R;
    cur = nxt;
    // nodes beyond the LDS mirror are read back from global memory by the next look-up
    if (nn > DEC_ARENA_LDS) __syncthreads();
    else lds_barrier();
  }
  __syncthreads();
  if constexpr (NBEST) {
    __shared__ int e_len[DEC_MAX_W], e_dup[DEC_MAX_W], e_src[DEC_MAX_W];
    __shared__ float e_sc[DEC_MAX_W], e_msc[DEC_MAX_W];
    __shared__ unsigned long long e_hash[DEC_MAX_W];
    const int N = nbest, n0 = min(N, nb);
    int* stage = w.cls + (long)slot * T * KS;  // row n: entry n's labels
    if constexpr (FUSED) {  // the final key adds the closing bigram: order the beams once more
      unsigned long long mine = 0ull;
      if (lane < nb) {
        const float close = f.lm ? f.weight * f.lm[(long)s_lab[cur][lane] * C] : 0.0f;
        mine = dec_ord(s_tot[cur][lane] + s_g[cur][lane] + close, lane);
        f_key[lane] = mine;
      }
      lds_barrier();
      if (lane < nb) {
        int rank = 0;
        for (int i = 0; i < nb; ++i) rank += f_key[i] > mine;
        p_src[rank] = lane;
      }
      lds_barrier();
    }
    int len = 0;
    if (lane < n0) {  // the active beams are in descending order of total: entry n is beam n
      auto node_at = [&](int n) { return n < DEC_ARENA_LDS ? a_lds[n] : arena[n]; };
      int beam = lane;
      if constexpr (FUSED) beam = p_src[lane];
      const int leaf = s_node[cur][beam];
      for (int n = leaf; len < Tb && dec_par(node_at(n)) >= 0; n = dec_par(node_at(n))) ++len;
      int* row = stage + (long)lane * T;
      int n = leaf;
      for (int i = len - 1; i >= 0; --i) {
        const unsigned long long nd = node_at(n);
        row[i] = dec_lab(nd);
        n = dec_par(nd);
      }
      unsigned long long h = 1469598103934665603ull;  // FNV-1a over the labels: a filter, not the comparison
      if (collapse) {
        int o = 0, prev = 0;
        for (int i = 0; i < len; ++i) {
          const int v = row[i];
          if (i == 0 || v != prev) {
            row[o++] = v;
            h = (h ^ (unsigned)v) * 1099511628211ull;
          }
          prev = v;
        }
        len = o;
      }
      e_len[lane] = len;
      e_hash[lane] = h;
      e_sc[lane] = (float)(offset + (double)s_tot[cur][beam]);
    }
    __syncthreads();  // the staged rows are read by other lanes below
    bool keep = lane < n0;
    float msc = keep ? e_sc[lane] : NEG_INF;
    if (collapse) {  // uncollapsed prefixes are distinct nodes and already sorted
      int dup = lane;
      if (lane < n0) {
        const int* mine = stage + (long)lane * T;
        for (int m = 0; m < lane && dup == lane; ++m) {  // the lowest earlier entry with equal labels
          if (e_len[m] != len || e_hash[m] != e_hash[lane]) continue;
          const int* other = stage + (long)m * T;
          bool eq = true;
          for (int i = 0; i < len; ++i) eq &= mine[i] == other[i];
          if (eq) dup = m;
        }
        e_dup[lane] = dup;
      }
      keep = lane < n0 && dup == lane;
      lds_barrier();
      if (keep)  // the survivor adds its duplicates in ascending entry order
        for (int m = lane + 1; m < n0; ++m)
          if (e_dup[m] == lane) msc = logaddexp_tail(msc, e_sc[m]);
    }
    if (lane < n0) e_msc[lane] = msc;
    const unsigned long long km = __ballot(keep);
    const int cnt = __popcll(km);
    lds_barrier();
    int rank = lane;
    if (collapse && keep) {  // stable: larger score first, ties to the lower entry
      const unsigned long long mine = dec_ord(msc, lane);
      rank = 0;
      for (int m = 0; m < n0; ++m) rank += ((km >> m) & 1ull) && dec_ord(e_msc[m], m) > mine;
    }
    if (keep) e_src[rank] = lane;
    lds_barrier();
    int* tok = tokens + (long)slot * N * T;
    for (int r = 0; r < N; ++r) {  // wave-uniform: every element of the clip's rows is written
      const int src = r < cnt ? e_src[r] : 0, ln = r < cnt ? e_len[src] : 0;
      const int* row = stage + (long)src * T;
      for (int i = lane; i < T; i += 64) tok[(long)r * T + i] = i < ln ? row[i] : 0;
    }
    if (lane < N) {
      const int src = lane < cnt ? e_src[lane] : 0;
      out_len[(long)slot * N + lane] = lane < cnt ? e_len[src] : 0;
      score[(long)slot * N + lane] = lane < cnt ? e_msc[src] : NEG_INF;
    }
    if (lane == 0) count[slot] = cnt;
    return;
  }
  // slot 0 is the best beam (ties to the lower slot); walk its prefix back to the root
  int* tok = tokens + (long)slot * T;
  if (lane == 0) {
    const int leaf = s_node[cur][0];
    int len = 0;
    for (int n = leaf; len < Tb && dec_par(arena[n]) >= 0; n = dec_par(arena[n])) ++len;
    int n = leaf;
    for (int i = len - 1; i >= 0; --i) {
      const unsigned long long nd = arena[n];
      tok[i] = dec_lab(nd);
      n = dec_par(nd);
    }
    if (collapse) {  // utils.py:185-188: groupby over the decoded labels
      int o = 0, prev = 0;
      for (int i = 0; i < len; ++i) {
        const int v = tok[i];
        if (i == 0 || v != prev) tok[o++] = v;
        prev = v;
      }
      len = o;
    }
    s_len = len;
    out_len[slot] = len;
    score[slot] = (float)(offset + (double)s_tot[cur][0]);
  }
  __syncthreads();
  for (int i = s_len + lane; i < T; i += 64) tok[i] = 0;
}

// One workgroup of 16 waves per (clip, head), grid (B, G): each wave takes every 16th frame's
// arg-max (ties to the lowest class; a frame is a chain of dependent loads, so frames run side
// by side), then wave 0 collapses repeats and drops blanks with a ballot scan.
constexpr int GREEDY_WAVES = 16;
__global__ __launch_bounds__(64 * GREEDY_WAVES) void ctc_greedy_kernel(CtcHeads hx,
                                                                        const int* __restrict__ in_len, DecDims d,
                                                                        int* __restrict__ tokens,
                                                                        int* __restrict__ out_len,
                                                                        float* __restrict__ score, DecWs w) {
  __shared__ float part[GREEDY_WAVES];
  __shared__ int s_len;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = (int)blockIdx.y * d.B + (int)blockIdx.x;
  const int T = d.T, C = d.C;
  const int Tb = clampi(in_len[blockIdx.x], 0, T);
  const float* __restrict__ x = ctc_head(hx, blockIdx.y) + (long)blockIdx.x * T * C;
  int* amax = w.cls + (long)slot * T;
  float acc = 0.0f;
  for (int t = wave; t < Tb; t += GREEDY_WAVES) {
    const long row = (long)slot * T + t;
    const float* xr = x + (long)t * C;
    float bv = NEG_INF;
    int bc = NONE;
    for (int c = lane; c < C; c += 64) {
      const float v = xr[c];
      if (v > bv) { bv = v; bc = c; }
    }
    wave_argmax(bv, bc);
    if (bc == NONE) bc = 0;
    if (lane == 0) amax[t] = bc;
    acc += ctc_lp_raw(xr[bc], w.rowstat[2 * row], w.rowstat[2 * row + 1]);
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  int* tok = tokens + (long)slot * T;
  if (wave == 0) {
    int count = 0;
    for (int base = 0; base < Tb; base += 64) {
      const int t = base + lane;
      const int a = t < Tb ? amax[t] : 0;
      const int prev = (t > 0 && t < Tb) ? amax[t - 1] : 0;
      const bool keep = t < Tb && a != 0 && (t == 0 || a != prev);
      const unsigned long long mask = __ballot(keep);
      if (keep) tok[count + __popcll(mask & ((1ull << lane) - 1ull))] = a;
      count += __popcll(mask);
    }
    if (lane == 0) {
      s_len = count;
      out_len[slot] = count;
      float sum = 0.0f;
      for (int i = 0; i < GREEDY_WAVES; ++i) sum += part[i];
      score[slot] = sum;
    }
  }
  __syncthreads();
  for (int i = s_len + tid; i < T; i += 64 * GREEDY_WAVES) tok[i] = 0;
}

// wer_pair, the alignment of one (reference, hypothesis) pair: wer_pair.h (shared with mwer.hip)
__global__ __launch_bounds__(128) void wer_kernel(const int* __restrict__ ref, const int* __restrict__ ref_len,
                                                  const int* __restrict__ hyp, const int* __restrict__ hyp_len,
                                                  int Rmax, int Hmax, int* __restrict__ counts) {
  const int n = blockIdx.x;
  const int R = clampi(ref_len[n], 0, Rmax), H = clampi(hyp_len[n], 0, Hmax);
  wer_pair(ref + (long)n * Rmax, R, hyp + (long)n * Hmax, H, counts + 4L * n);
}

struct EvalLog {
  int* hyp;      // (capacity, G, width) or NULL
  int* hyp_len;  // (capacity, G)
  int capacity, width;
};

// Launch 1 of sca_eval_accumulate, grid (B, G): the pair (reference b, head g's hypothesis of
// clip b).  The references are indexed by clip, not tiled over the heads.  cursor is read
// here and advanced by launch 2, which the stream orders behind every workgroup of this one.
__global__ __launch_bounds__(128) void eval_score_kernel(const int* __restrict__ tokens,
                                                         const int* __restrict__ hyp_len, int Hmax,
                                                         const int* __restrict__ ref, const int* __restrict__ ref_len,
                                                         int Rmax, int* __restrict__ counts, sca_eval_state* state,
                                                         EvalLog log) {
  const int b = blockIdx.x, g = blockIdx.y, B = gridDim.x, G = gridDim.y, tid = threadIdx.x;
  const long n = (long)g * B + b;
  const int R = clampi(ref_len[b], 0, Rmax), H = clampi(hyp_len[n], 0, Hmax);
  const int* hrow = tokens + n * Hmax;
  int* out = counts + 4 * n;
  wer_pair(ref + (long)b * Rmax, R, hrow, H, out);
  if (tid == 0) {  // integer adds commute: the totals do not depend on the order of arrival
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(&state->totals[g][k], out[k]);
  }
  if (log.hyp) {
    const long row = (long)state->cursor + b;
    if (row < log.capacity) {
      int* dst = log.hyp + (row * G + g) * log.width;
      for (int i = tid; i < log.width; i += 128) dst[i] = i < H ? hrow[i] : 0;
      if (tid == 0) log.hyp_len[row * G + g] = min(H, log.width);
      if (tid == 0 && H > log.width) atomicOr(&state->overflow, SCA_EVAL_LOG_TRUNCATED);
    } else if (tid == 0) {
      atomicOr(&state->overflow, SCA_EVAL_LOG_DROPPED);
    }
  }
}

// Launch 2, one wave: the step's report into the pass's sums, then the cursor moves on.
__global__ __launch_bounds__(64) void eval_advance_kernel(const unsigned* __restrict__ report, int nflags, int nloss,
                                                          int B, sca_eval_state* state) {
  const int lane = threadIdx.x;
  unsigned any = 0;
  for (int i = lane; i < nflags; i += 64) {
    const unsigned f = report[i];
    if (f) state->flags[i] |= f;
    any |= f;
  }
  const bool flagged = __any(any != 0);
  if (lane < nloss) state->loss_sum[lane] += (double)__uint_as_float(report[nflags + lane]);
  if (lane == 0) {
    const int steps = state->steps;
    if (flagged && state->first_flagged == 0) state->first_flagged = steps + 1;
    state->steps = steps + 1;
    state->cursor += B;
  }
}

// ---- the second pass over an n-best list (include/scatten.h): rescoring, posterior, MBR ----
// One wave per (head, clip).  The lanes stride over the len + 1 bigram terms of one entry at a
// time (independent gathers), a butterfly sums them; lane n then holds entry n's total for the
// softmax over the valid entries and the rank count that gives `order`.
// Prior: the gloss model as a functor of ctc.h, the dense table or the backoff trie.
template <class Prior>
__global__ __launch_bounds__(64) void nbest_rescore_kernel(const int* __restrict__ tokens,
                                                           const int* __restrict__ out_len,
                                                           const float* __restrict__ score,
                                                           const int* __restrict__ count, int N, int T, Prior prior,
                                                           float lm_weight, float length_bonus, float posterior_scale,
                                                           float* __restrict__ total, float* __restrict__ posterior,
                                                           int* __restrict__ order) {
  __shared__ unsigned long long key[DEC_MAX_W];
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int cnt = clampi(count[s], 0, N);
  float mine = NEG_INF;
  for (int n = 0; n < cnt; ++n) {
    const int len = clampi(out_len[s * N + n], 0, T);
    const int* h = tokens + (s * N + n) * T;
    const float t = score[s * N + n] + prior(h, len, lane, lm_weight, length_bonus);
    mine = lane == n ? t : mine;
  }
  const bool valid = lane < cnt;
  const float z = valid ? posterior_scale * mine : NEG_INF;
  const float m = wave_max(z);
  const float e = valid ? expf(z - m) : 0.0f;
  const float sum = wave_sum(e);
  if (lane < N) {
    total[s * N + lane] = valid ? mine : NEG_INF;
    posterior[s * N + lane] = valid ? e / sum : 0.0f;
    key[lane] = valid ? dec_ord(mine, lane) : 0ull;
  }
  lds_barrier();
  if (valid) {  // the keys are distinct: the ranks are a permutation of [0, cnt)
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += key[j] > key[lane];
    order[s * N + rank] = lane;
  } else if (lane < N) {
    order[s * N + lane] = lane;
  }
}

// MBR launch 1, grid (G B, N N): loss[i, j] of the ordered pair (hypothesis i, reference j) of
// one (head, clip); 0 on the diagonal and where either entry is not valid.
__global__ __launch_bounds__(128) void nbest_loss_kernel(const int* __restrict__ tokens,
                                                         const int* __restrict__ out_len,
                                                         const int* __restrict__ count, int N, int T,
                                                         int* __restrict__ loss) {
  __shared__ int c4[4];
  const long s = blockIdx.x;
  const int i = (int)blockIdx.y / N, j = (int)blockIdx.y - i * N;
  const int cnt = clampi(count[s], 0, N);
  int* out = loss + (s * N + i) * N + j;
  if (i == j || i >= cnt || j >= cnt) {  // uniform over the workgroup
    if (threadIdx.x == 0) *out = 0;
    return;
  }
  const int R = clampi(out_len[s * N + j], 0, T), H = clampi(out_len[s * N + i], 0, T);
  wer_pair(tokens + (s * N + j) * T, R, tokens + (s * N + i) * T, H, c4);
  if (threadIdx.x == 0) *out = c4[0] + c4[1] + c4[2];  // thread 0 wrote c4
}

// MBR launch 2, one wave per (head, clip): lane i sums its row in ascending j, then the arg-min
// (ties to the lower entry).
__global__ __launch_bounds__(64) void nbest_risk_kernel(const int* __restrict__ loss,
                                                        const float* __restrict__ posterior,
                                                        const int* __restrict__ count, int N,
                                                        float* __restrict__ risk, int* __restrict__ best) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int cnt = clampi(count[s], 0, N);
  const bool valid = lane < cnt;
  float r = 0.0f;
  if (valid)
    for (int j = 0; j < cnt; ++j) r += posterior[s * N + j] * (float)loss[(s * N + lane) * N + j];
  float v = valid ? r : -NEG_INF;
  if (lane < N) risk[s * N + lane] = v;
  int idx = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o, 64);
    const int d = __shfl_xor(idx, o, 64);
    if (w < v || (w == v && d < idx)) { v = w; idx = d; }
  }
  if (lane == 0) best[s] = clampi(idx, 0, max(cnt - 1, 0));
}

// One wave per (head, clip): entry sel[s * sel_stride] of the list as a 1-best-shaped row.
__global__ __launch_bounds__(64) void nbest_gather_kernel(const int* __restrict__ tokens,
                                                          const int* __restrict__ out_len,
                                                          const float* __restrict__ value,
                                                          const int* __restrict__ sel, int sel_stride, int N, int T,
                                                          int* __restrict__ tokens1, int* __restrict__ out_len1,
                                                          float* __restrict__ value1) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int e = clampi(sel[s * sel_stride], 0, N - 1);
  const int len = clampi(out_len[s * N + e], 0, T);
  const int* row = tokens + (s * N + e) * T;
  for (int i = lane; i < T; i += 64) tokens1[s * T + i] = i < len ? row[i] : 0;
  if (lane == 0) {
    out_len1[s] = len;
    value1[s] = value[s * N + e];
  }
}

bool nbest_dims_ok(int G, int B, int N, int T) {
  return G >= 1 && G <= SCA_EVAL_MAX_HEADS && B >= 1 && (long)G * B <= 0x7fffffffL / 4 && N >= 1 && N <= DEC_MAX_W &&
         T >= 1;
}

bool dec_dims_ok(int B, int T, int C, int W) {
  return B >= 1 && T >= 1 && C >= 1 && C <= SCA_CTC_MAX_C && W >= 1 && W <= SCA_CTC_MAX_BEAM;
}

// G B clips must stay countable in an int (the kernels' slot index)
bool dec_heads_ok(const sca_decode_heads* heads, int G, int B, int T, int C, int W) {
  if (G < 1 || G > SCA_EVAL_MAX_HEADS || !dec_dims_ok(B, T, C, W) || (long)G * B > 0x7fffffffL / 4 || !heads)
    return false;
  for (int g = 0; g < G; ++g)
    if (!heads->logits[g]) return false;
  return true;
}

// the single-head layout over N = G B clips; 0 for unsupported sizes
long dec_ws_bytes(int G, int B, int T, int C, int W) {
  if (G < 1 || G > SCA_EVAL_MAX_HEADS || !dec_dims_ok(B, T, C, W)) return 0;
  const long N = (long)G * B, NT = N * T;
  return 4 * (2 * NT + 2 * NT * (W + 1)) + 8 * N * ((long)T * W + 1);
}

// One call of any of the eight decoders.  A single-head entry point is G = 1 with its tensor in
// heads->logits[0]; the fields a mode does not take are 0 / NULL.
enum DecMode { DEC_GREEDY, DEC_BEAM, DEC_NBEST, DEC_FUSED };
struct DecCall {
  DecMode mode;
  const sca_decode_heads* heads;
  int G;
  const int* in_len;
  DecDims d;            // W = beam_width; 1 for DEC_GREEDY
  int collapse, nbest;  // nbest, count: DEC_NBEST and DEC_FUSED
  DecLm f;              // DEC_FUSED
  int *tokens, *out_len;
  float* score;
  int* count;
  void* ws;
};

bool dec_call_ok(const DecCall& c) {
  if (!dec_heads_ok(c.heads, c.G, c.d.B, c.d.T, c.d.C, c.d.W) || !c.in_len || !c.tokens || !c.out_len || !c.score ||
      !c.ws)
    return false;
  if (c.mode >= DEC_NBEST && (c.nbest < 1 || c.nbest > c.d.W || !c.count)) return false;
  return c.mode != DEC_FUSED || (c.f.weight - c.f.weight == 0.0f && c.f.bonus - c.f.bonus == 0.0f);
}

// The launches of every decoder: the row statistics of all G B T rows, the per-frame best labels
// (the fused search selects its own per beam, the greedy kernel needs none), then one workgroup
// per (clip, head).
void dec_launch(const DecCall& c, hipStream_t st) {
  const DecDims d = c.d;
  const DecWs w(c.ws, d, c.G);
  const CtcHeads hx = ctc_heads_of(c.heads, c.G);
  const long rows = (long)c.G * d.B * d.T;
  const dim3 clips(d.B, c.G);
  // one tensor: the CTC loss's launch of the same row body, without the head select (measured:
  // 0.2 us of the 24 us greedy decode at B = 8, T = 64, C = 1124)
  if (c.G == 1) sca_ctc_rowstat_launch(c.heads->logits[0], w.rowstat, rows, d.C, st);
  else sca_ctc_rowstat_heads_launch(c.heads, c.G, w.rowstat, (long)d.B * d.T, d.C, st);
  if (c.mode == DEC_BEAM || c.mode == DEC_NBEST)
    hipLaunchKernelGGL(ctc_topk_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, hx, c.G, c.in_len, d, w);
  if (c.mode == DEC_GREEDY) {
    hipLaunchKernelGGL(ctc_greedy_kernel, clips, dim3(64 * GREEDY_WAVES), 0, st, hx, c.in_len, d, c.tokens, c.out_len,
                       c.score, w);
    return;
  }
  const auto search = c.mode == DEC_BEAM    ? ctc_beam_kernel<false>
                      : c.mode == DEC_NBEST ? ctc_beam_kernel<true>
                                            : ctc_beam_kernel<true, true>;
  hipLaunchKernelGGL(search, clips, dim3(64), 0, st, hx, c.in_len, d, c.collapse, c.nbest, c.tokens, c.out_len,
                     c.score, c.count, w, c.f);
}

// An entry point: the argument check, the launches, the launch check.  `name` and `grouped`
// (the _heads form) only word the messages.
int dec_decode(const char* name, bool grouped, const DecCall& c, void* stream) {
  static const char* const limits[] = {"", ", 1 <= beam_width <= 32", ", 1 <= nbest <= beam_width <= 32",
                                       ", 1 <= nbest <= beam_width <= 32, finite weights"};
  if (!dec_call_ok(c)) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: bad arguments (%sB, T >= 1, 1 <= C <= 8192%s)", name,
             grouped ? "1 <= G <= 8 non-null tensors, " : "", limits[c.mode]);
    sca_set_error(msg);
    return SCA_ERR_ARG;
  }
  dec_launch(c, reinterpret_cast<hipStream_t>(stream));
  return sca_launch_status(name);
}

}  // namespace

// the row max / log-sum-exp pass of G heads (ctc.h)
void sca_ctc_rowstat_heads_launch(const sca_decode_heads* heads, int G, float* rowstat, long rows_per_head, int C,
                                  hipStream_t st) {
  const long rows = (long)G * rows_per_head;
  hipLaunchKernelGGL(ctc_rowstat_heads_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                     ctc_heads_of(heads, G), rowstat, rows, rows_per_head, C);
}

extern "C" long sca_ctc_decode_workspace_bytes(int B, int T, int C, int W) { return dec_ws_bytes(1, B, T, C, W); }

extern "C" long sca_ctc_decode_heads_workspace_bytes(int G, int B, int T, int C, int W) {
  return dec_ws_bytes(G, B, T, C, W);
}

// the same layout; cls holds the tail's rows only
extern "C" long sca_ctc_fused_workspace_bytes(int G, int B, int T, int C, int W) { return dec_ws_bytes(G, B, T, C, W); }

extern "C" int sca_ctc_greedy_decode(const float* logits, const int* in_len, int B, int T, int C, int* tokens,
                                     int* out_len, float* score, void* ws, void* stream) {
  const sca_decode_heads one = {{logits}};
  return dec_decode("sca_ctc_greedy_decode", false,
                    {DEC_GREEDY, &one, 1, in_len, {B, T, C, 1}, 0, 0, {}, tokens, out_len, score, nullptr, ws}, stream);
}

extern "C" int sca_ctc_beam_decode(const float* logits, const int* in_len, int B, int T, int C, int beam_width,
                                   int collapse_repeats, int* tokens, int* out_len, float* score, void* ws,
                                   void* stream) {
  const sca_decode_heads one = {{logits}};
  return dec_decode("sca_ctc_beam_decode", false,
                    {DEC_BEAM, &one, 1, in_len, {B, T, C, beam_width}, collapse_repeats != 0, 0, {}, tokens, out_len,
                     score, nullptr, ws},
                    stream);
}

extern "C" int sca_ctc_greedy_decode_heads(const sca_decode_heads* heads, int G, const int* in_len, int B, int T,
                                           int C, int* tokens, int* out_len, float* score, void* ws, void* stream) {
  return dec_decode("sca_ctc_greedy_decode_heads", true,
                    {DEC_GREEDY, heads, G, in_len, {B, T, C, 1}, 0, 0, {}, tokens, out_len, score, nullptr, ws},
                    stream);
}

extern "C" int sca_ctc_beam_decode_heads(const sca_decode_heads* heads, int G, const int* in_len, int B, int T, int C,
                                         int beam_width, int collapse_repeats, int* tokens, int* out_len, float* score,
                                         void* ws, void* stream) {
  return dec_decode("sca_ctc_beam_decode_heads", true,
                    {DEC_BEAM, heads, G, in_len, {B, T, C, beam_width}, collapse_repeats != 0, 0, {}, tokens, out_len,
                     score, nullptr, ws},
                    stream);
}

extern "C" int sca_wer_counts(const int* ref, const int* ref_len, const int* hyp, const int* hyp_len, int N,
                              int Rmax, int Hmax, int* counts, void* stream) {
  if (N < 1 || Rmax < 0 || Rmax > SCA_WER_MAX_LEN || Hmax < 0 || Hmax > SCA_WER_MAX_LEN || !ref_len || !hyp_len ||
      (Rmax > 0 && !ref) || (Hmax > 0 && !hyp) || !counts) {
    sca_set_error("sca_wer_counts: bad arguments (N >= 1, 0 <= Rmax, Hmax <= 128)");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(wer_kernel, dim3(N), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), ref, ref_len, hyp,
                     hyp_len, Rmax, Hmax, counts);
  return sca_launch_status("sca_wer_counts");
}

extern "C" int sca_eval_accumulate(const int* tokens, const int* hyp_len, int G, int B, int Hmax, const int* ref,
                                   const int* ref_len, int Rmax, const void* report, int nflags, int nloss,
                                   int* counts, sca_eval_state* state, int* hyp_log, int* hyp_len_log, int capacity,
                                   int log_width, void* stream) {
  const bool log = capacity > 0;
  if (G < 1 || G > SCA_EVAL_MAX_HEADS || B < 1 || Rmax < 0 || Rmax > SCA_WER_MAX_LEN || Hmax < 0 ||
      Hmax > SCA_WER_MAX_LEN || nflags < 0 || nflags > SCA_REPORT_MAX_FLAGS || nloss < 0 ||
      nloss > SCA_EVAL_MAX_LOSSES || capacity < 0 || !hyp_len || !ref_len || (Rmax > 0 && !ref) ||
      (Hmax > 0 && !tokens) || !report || !counts || !state || (log && (!hyp_log || !hyp_len_log || log_width < 1))) {
    sca_set_error("sca_eval_accumulate: bad arguments (1 <= G <= 8, B >= 1, 0 <= Rmax, Hmax <= 128, "
                  "nflags <= 64, nloss <= 11, a log needs hyp_log, hyp_len_log and log_width >= 1)");
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const EvalLog lg{log ? hyp_log : nullptr, log ? hyp_len_log : nullptr, capacity, log_width};
  hipLaunchKernelGGL(eval_score_kernel, dim3(B, G), dim3(128), 0, st, tokens, hyp_len, Hmax, ref, ref_len, Rmax, counts,
                     state, lg);
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(64), 0, st, static_cast<const unsigned*>(report), nflags, nloss,
                     B, state);
  return sca_launch_status("sca_eval_accumulate");
}

extern "C" int sca_ctc_beam_decode_nbest(const float* logits, const int* in_len, int B, int T, int C, int beam_width,
                                         int nbest, int collapse_repeats, int* tokens, int* out_len, float* score,
                                         int* count, void* ws, void* stream) {
  const sca_decode_heads one = {{logits}};
  return dec_decode("sca_ctc_beam_decode_nbest", false,
                    {DEC_NBEST, &one, 1, in_len, {B, T, C, beam_width}, collapse_repeats != 0, nbest, {}, tokens,
                     out_len, score, count, ws},
                    stream);
}

extern "C" int sca_ctc_beam_decode_heads_nbest(const sca_decode_heads* heads, int G, const int* in_len, int B, int T,
                                               int C, int beam_width, int nbest, int collapse_repeats, int* tokens,
                                               int* out_len, float* score, int* count, void* ws, void* stream) {
  return dec_decode("sca_ctc_beam_decode_heads_nbest", true,
                    {DEC_NBEST, heads, G, in_len, {B, T, C, beam_width}, collapse_repeats != 0, nbest, {}, tokens,
                     out_len, score, count, ws},
                    stream);
}

// shallow fusion: the bigram model inside the search (include/scatten.h)
extern "C" int sca_ctc_beam_decode_fused_nbest(const float* logits, const int* in_len, int B, int T, int C,
                                               int beam_width, int nbest, int collapse_repeats, const float* lm,
                                               float lm_weight, float length_bonus, int* tokens, int* out_len,
                                               float* score, int* count, void* ws, void* stream) {
  const sca_decode_heads one = {{logits}};
  return dec_decode("sca_ctc_beam_decode_fused_nbest", false,
                    {DEC_FUSED, &one, 1, in_len, {B, T, C, beam_width}, collapse_repeats != 0, nbest,
                     {lm, lm_weight, length_bonus}, tokens, out_len, score, count, ws},
                    stream);
}

extern "C" int sca_ctc_beam_decode_heads_fused_nbest(const sca_decode_heads* heads, int G, const int* in_len, int B,
                                                     int T, int C, int beam_width, int nbest, int collapse_repeats,
                                                     const float* lm, float lm_weight, float length_bonus,
                                                     int* tokens, int* out_len, float* score, int* count, void* ws,
                                                     void* stream) {
  return dec_decode("sca_ctc_beam_decode_heads_fused_nbest", true,
                    {DEC_FUSED, heads, G, in_len, {B, T, C, beam_width}, collapse_repeats != 0, nbest,
                     {lm, lm_weight, length_bonus}, tokens, out_len, score, count, ws},
                    stream);
}

extern "C" int sca_nbest_rescore(const int* tokens, const int* out_len, const float* score, const int* count, int G,
                                 int B, int N, int T, const float* lm, int C, float lm_weight, float length_bonus,
                                 float posterior_scale, float* total, float* posterior, int* order, void* stream) {
  if (!nbest_dims_ok(G, B, N, T) || !tokens || !out_len || !score || !count || !total || !posterior || !order ||
      (lm && (C < 1 || C > SCA_CTC_MAX_C)) || !(lm_weight - lm_weight == 0.0f) ||
      !(length_bonus - length_bonus == 0.0f) || !(posterior_scale - posterior_scale == 0.0f)) {
    sca_set_error("sca_nbest_rescore: bad arguments (1 <= G <= 8, B, T >= 1, 1 <= N <= 32, 1 <= C <= 8192 with a "
                  "table, finite weights)");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(nbest_rescore_kernel<CtcBigramPrior>, dim3((unsigned)(G * B)), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), tokens, out_len, score, count, N, T, CtcBigramPrior{lm, C},
                     lm_weight, length_bonus, posterior_scale, total, posterior, order);
  return sca_launch_status("sca_nbest_rescore");
}

extern "C" int sca_nbest_rescore_ngram(const int* tokens, const int* out_len, const float* score, const int* count,
                                       int G, int B, int N, int T, const sca_ngram_lm* lm, float lm_weight,
                                       float length_bonus, float posterior_scale, float* total, float* posterior,
                                       int* order, void* stream) {
  if (!nbest_dims_ok(G, B, N, T) || !tokens || !out_len || !score || !count || !total || !posterior || !order ||
      !ctc_ngram_ok(lm) || !(lm_weight - lm_weight == 0.0f) || !(length_bonus - length_bonus == 0.0f) ||
      !(posterior_scale - posterior_scale == 0.0f)) {
    sca_set_error("sca_nbest_rescore_ngram: bad arguments (1 <= G <= 8, B, T >= 1, 1 <= N <= 32; with a model: order "
                  "in 1..3, 1 <= C <= 8192, counts >= 0, the arrays of the orders in use; finite weights)");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(nbest_rescore_kernel<CtcNgramPrior>, dim3((unsigned)(G * B)), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), tokens, out_len, score, count, N, T,
                     CtcNgramPrior{ctc_ngram_of(lm)}, lm_weight, length_bonus, posterior_scale, total, posterior,
                     order);
  return sca_launch_status("sca_nbest_rescore_ngram");
}

extern "C" int sca_nbest_mbr(const int* tokens, const int* out_len, const int* count, const float* posterior, int G,
                             int B, int N, int T, int* loss, float* risk, int* best, void* stream) {
  if (!nbest_dims_ok(G, B, N, T) || T > SCA_WER_MAX_LEN || !tokens || !out_len || !count || !posterior || !loss ||
      !risk || !best) {
    sca_set_error("sca_nbest_mbr: bad arguments (1 <= G <= 8, B >= 1, 1 <= N <= 32, 1 <= T <= 128)");
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(nbest_loss_kernel, dim3((unsigned)(G * B), (unsigned)(N * N)), dim3(128), 0, st, tokens, out_len,
                     count, N, T, loss);
  hipLaunchKernelGGL(nbest_risk_kernel, dim3((unsigned)(G * B)), dim3(64), 0, st, loss, posterior, count, N, risk,
                     best);
  return sca_launch_status("sca_nbest_mbr");
}

extern "C" int sca_nbest_gather(const int* tokens, const int* out_len, const float* value, const int* sel,
                                int sel_stride, int G, int B, int N, int T, int* tokens1, int* out_len1,
                                float* value1, void* stream) {
  if (!nbest_dims_ok(G, B, N, T) || sel_stride < 1 || sel_stride > N || !tokens || !out_len || !value || !sel ||
      !tokens1 || !out_len1 || !value1) {
    sca_set_error("sca_nbest_gather: bad arguments (1 <= G <= 8, B, T >= 1, 1 <= N <= 32, 1 <= sel_stride <= N)");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(nbest_gather_kernel, dim3((unsigned)(G * B)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                     tokens, out_len, value, sel, sel_stride, N, T, tokens1, out_len1, value1);
  return sca_launch_status("sca_nbest_gather");
}
