// Minimum word error rate (MWER) training loss over an n-best list (include/scatten.h): the
// expected number of errors of the list's hypotheses under the model's own posterior over the
// list, with exact CTC likelihoods, and its gradient with respect to the logits.  The reference
// has none of this.
//   fwd: row statistics (the pass the CTC loss and the decoders share) -> one launch with alpha
//        and beta of every (clip, slot), one wave64 each, beside its error count, the alignment
//        of wer_pair.h, and its prior under the gloss model -> posterior, centred errors,
//        gradient weights, risk, loss
//   bwd: one workgroup per (clip, frame): sum_n w_n occ_n(t, .) in one LDS row, n ascending,
//        then the clamp gate and the log-softmax backward: ONE dense pass for the M slots
// One set of kernels behind sca_mwer_fwd / bwd and sca_mwer_heads_fwd / bwd.  A "clip" of the
// grids, the workspace and the outputs is the (head, clip) pair p = g B + b (CtcHeads, ctc.h);
// a slot is an entry of the list or, with_ref, slot N: the clip's reference, read where it lies
// (no copy of the list).  One host path too (MwCall): sca_mwer_fwd / bwd are its G = 1 case
// without the reference and the prior, and a heads call without a table and a length bonus
// skips the prior as they do.
// No float atomics; every sum over slots, states and clips runs in a fixed order, so the
// results are deterministic and a replayed capture is bitwise the eager call.
#include "ctc.h"
#include "wer_pair.h"

namespace {

constexpr int MW_MAX_L = 2 * SCA_WER_MAX_LEN + 1;  // states of the longest hypothesis
constexpr int MW_K = (MW_MAX_L + 63) / 64;         // states per lane of the recursion's wave
constexpr int MW_PAD = 2;                          // -inf cells either side of an LDS state row
constexpr int MW_GRAD_THREADS = 256;
constexpr int MW_CLIPS_ONE_GROUP = 64;  // up to this many (head, clip) pairs: per-clip statistics and the losses in one workgroup

// B clips per head, P = G B pairs; N entries and M = N + with_ref slots per pair; Hm = the longest
// labelling of a slot (H, or max(H, R) with the reference); prior: lmterm is computed and added
struct MwDims {
  int B, N, T, C, H, R, P, M, Hm, with_ref, prior;
};

MwDims mw_dims(int G, int B, int N, int T, int C, int H, int R, int with_ref, int prior) {
  return MwDims{B, N, T, C, H, R, G * B, N + (with_ref ? 1 : 0), with_ref && R > H ? R : H, with_ref ? 1 : 0, prior};
}

// The gloss model of the prior (sca_nbest_rescore's arguments); Prior: the functor of ctc.h, the
// dense table (MwPrior, what the call record holds) or the backoff trie
template <class Prior>
struct MwPriorOf {
  Prior lm;
  float weight, bonus;
};
struct MwPrior {
  const float* lm;
  float weight, bonus;
};

// d loss / d logits of the G heads, by value in the kernel arguments like CtcHeads
struct MwGrads {
  float* dx[SCA_EVAL_MAX_HEADS];
};

__device__ __forceinline__ float* mw_grad_head(const MwGrads& h, int g) {
  float* p = h.dx[0];
#pragma unroll
  for (int i = 1; i < SCA_EVAL_MAX_HEADS; ++i) p = g == i ? h.dx[i] : p;
  return p;
}

// workspace layout (floats): rowstat[P T 2] | alpha[P M T Lm] | beta[P M T Lm] | ll[P M] |
// w[P M] | lossb[P] | lmterm[P M] (with the prior only), Lm = 2 Hm + 1
struct MwWs {
  float *rowstat, *alpha, *beta, *ll, *w, *lossb, *lmterm;
  long Lm;
  __host__ __device__ MwWs(float* ws, MwDims d) {
    const long PT = (long)d.P * d.T, PM = (long)d.P * d.M;
    Lm = 2L * d.Hm + 1;
    rowstat = ws;
    alpha = rowstat + 2 * PT;
    beta = alpha + PM * d.T * Lm;
    ll = beta + PM * d.T * Lm;
    w = ll + PM;
    lossb = w + PM;
    lmterm = lossb + d.P;
  }
};

long mw_ws_floats(long P, long M, long T, long Hm, bool prior) {
  return 2 * P * T + 2 * P * M * T * (2 * Hm + 1) + 2 * P * M + P + (prior ? P * M : 0);
}

// The labelling of slot n of pair p: entry n of the list, or (n = N) the reference of clip b
struct MwSlot {
  const int* tok;
  int len;
};

__device__ __forceinline__ MwSlot mw_slot(const int* __restrict__ tokens, const int* __restrict__ out_len,
                                          const int* __restrict__ ref, const int* __restrict__ ref_len, MwDims d,
                                          int p, int b, int n) {
  if (n == d.N) return MwSlot{ref + (long)b * d.R, clampi(ref_len[b], 0, d.R)};
  const long el = (long)p * d.N + n;
  return MwSlot{tokens + el * d.H, clampi(out_len[el], 0, d.H)};
}

// One wave64 per (slot, pair, direction) of mwer_entry_kernel: z = 0 the alpha recursion over
// the frames [0, in_len), z = 1 the beta one.  Lane l holds states l, l + 64, ..; a frame's row
// goes through a wave-private LDS row for the neighbours s -+ 1, s -+ 2, so a frame costs no
// workgroup barrier.  The emissions lp[t, label(s)] do not depend on the recursion: the next
// frame's gathers are issued before this frame's row is computed.
__device__ __forceinline__ void mwer_alpha_beta(const CtcHeads& heads, const int* __restrict__ in_len,
                                                const int* __restrict__ tokens, const int* __restrict__ out_len,
                                                const int* __restrict__ count, const int* __restrict__ ref,
                                                const int* __restrict__ ref_len, MwDims d, float* ws) {
  __shared__ float buf[2][MW_MAX_L + 2 * MW_PAD];
  MwWs w(ws, d);
  const int n = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
  const int g = p / d.B, b = p - g * d.B;
  const bool beta_pass = blockIdx.z == 1;
  const long e = (long)p * d.M + n;
  const int cnt = clampi(count[p], 0, d.N);
  const int Tb = clampi(in_len[b], 0, d.T);
  if (n < d.N && n >= cnt) {  // uniform: entries past count are ignored
    if (!beta_pass && lane == 0) w.ll[e] = NEG_INF;
    return;
  }
  const MwSlot slot = mw_slot(tokens, out_len, ref, ref_len, d, p, b, n);
  const int len = slot.len;
  if (Tb == 0) {  // no frame: only the empty hypothesis fits, with likelihood 1
    if (!beta_pass && lane == 0) w.ll[e] = len == 0 ? 0.0f : NEG_INF;
    return;
  }
  const int L = 2 * len + 1;
  const int* tok = slot.tok;
  int lab[MW_K];
  bool skip[MW_K];  // the transition from s - 2 (alpha) / s + 2 (beta) exists
#pragma unroll
  for (int k = 0; k < MW_K; ++k) {
    const int s = lane + 64 * k;
    lab[k] = 0;
    skip[k] = false;
    if (s < L && (s & 1)) {
      const int j = (s - 1) >> 1;
      lab[k] = clampi(tok[j], 0, d.C - 1);
      // a token equal to the blank (no decoder emits one) is a blank state: no skip into it
      if (!beta_pass && j >= 1) skip[k] = lab[k] != 0 && clampi(tok[j - 1], 0, d.C - 1) != lab[k];
      if (beta_pass && j + 1 < len) skip[k] = lab[k] != 0 && clampi(tok[j + 1], 0, d.C - 1) != lab[k];
    }
  }
  const float* xb = ctc_head(heads, g) + (long)b * d.T * d.C;
  const float* rs = w.rowstat + 2L * p * d.T;
  float* out = (beta_pass ? w.beta : w.alpha) + e * d.T * w.Lm;
  auto emit = [&](int t, int k) {
    return ctc_lp(ctc_lp_raw(xb[(long)t * d.C + lab[k]], rs[2 * t], rs[2 * t + 1]));
  };
  if (lane < MW_PAD) {
    buf[0][lane] = buf[1][lane] = NEG_INF;
    buf[0][MW_PAD + L + lane] = buf[1][MW_PAD + L + lane] = NEG_INF;
  }
  const int t0 = beta_pass ? Tb - 1 : 0, dt = beta_pass ? -1 : 1, nb = beta_pass ? 1 : -1;
  float ec[MW_K], en[MW_K];
#pragma unroll
  for (int k = 0; k < MW_K; ++k) {
    const int s = lane + 64 * k;
    ec[k] = 0.0f;
    if (s < L) {
      const bool on = beta_pass ? s >= L - 2 : s < 2;
      const float v = on ? emit(t0, k) : NEG_INF;
      buf[0][MW_PAD + s] = v;
      out[(long)t0 * w.Lm + s] = v;
      if (Tb > 1) ec[k] = emit(t0 + dt, k);
    }
  }
  int cur = 0;
  for (int step = 1; step < Tb; ++step) {
    const int t = t0 + dt * step;
    const bool more = step + 1 < Tb;
#pragma unroll
    for (int k = 0; k < MW_K; ++k) {
      en[k] = 0.0f;
      if (more && lane + 64 * k < L) en[k] = emit(t + dt, k);
    }
    wave_lds_sync();
    const float* prev = buf[cur] + MW_PAD;
    float* nxt = buf[cur ^ 1] + MW_PAD;
#pragma unroll
    for (int k = 0; k < MW_K; ++k) {
      const int s = lane + 64 * k;
      if (s < L) {
        const float a1 = prev[s], a2 = prev[s + nb];
        const float a3 = skip[k] ? prev[s + 2 * nb] : NEG_INF;
        const float v = lse3(a1, a2, a3) + ec[k];
        nxt[s] = v;
        out[(long)t * w.Lm + s] = v;
      }
      ec[k] = en[k];
    }
    cur ^= 1;
  }
  wave_lds_sync();
  if (!beta_pass && lane == 0) {
    // ll = log(exp(alpha[Tb-1][L-1]) + exp(alpha[Tb-1][L-2])); the pad cell is -inf for L = 1
    w.ll[e] = ctc_end_loglik(buf[cur][MW_PAD + L - 1], buf[cur][MW_PAD + L - 2]);  // -inf: the hypothesis does not fit
  }
}

// z = 2 of mwer_entry_kernel, one workgroup per (slot, pair): errors[p, n] = num_del + num_ins +
// num_sub of reference b against entry n; 0 for the entries past count and for the reference
// slot, which needs no alignment.  With the prior, wave 1 computes the slot's lmterm once it has
// left wer_pair's last barrier, beside thread 0's serial back-trace.
template <class Prior>
__device__ __forceinline__ void mwer_pair(const int* __restrict__ tokens, const int* __restrict__ out_len,
                                          const int* __restrict__ count, const int* __restrict__ ref,
                                          const int* __restrict__ ref_len, MwDims d, const MwPriorOf<Prior>& prior,
                                          float* ws, int* __restrict__ errors) {
  __shared__ int c4[4];
  const int n = blockIdx.x, p = blockIdx.y;
  const int b = p % d.B;
  const long e = (long)p * d.M + n;
  const bool listed = n < clampi(count[p], 0, d.N);  // uniform over the workgroup
  if (listed) {
    const long el = (long)p * d.N + n;
    const int R = clampi(ref_len[b], 0, d.R), H = clampi(out_len[el], 0, d.H);
    wer_pair(ref + (long)b * d.R, R, tokens + el * d.H, H, c4);
    if (threadIdx.x == 0) errors[e] = c4[0] + c4[1] + c4[2];  // thread 0 wrote c4
  } else if (threadIdx.x == 0) {
    errors[e] = 0;
  }
  if (d.prior && threadIdx.x >= 64) {
    const int lane = threadIdx.x - 64;
    float v = 0.0f;
    if (listed || n == d.N) {
      const MwSlot slot = mw_slot(tokens, out_len, ref, ref_len, d, p, b, n);
      v = prior.lm(slot.tok, slot.len, lane, prior.weight, prior.bonus);
    }
    if (lane == 0) MwWs(ws, d).lmterm[e] = v;
  }
}

// grid (M, P, 3), 128 threads: the three independent jobs of one (slot, pair) in ONE launch, so
// that the alignment (an anti-diagonal sweep and a serial back-trace) and the prior run beside
// the two recursions instead of after them.  z = 0, 1: wave 0 runs the recursion, wave 1 leaves
// at once (the recursion uses no workgroup barrier); z = 2: both waves run wer_pair.
template <class Prior>
__global__ __launch_bounds__(128) void mwer_entry_kernel(CtcHeads heads, const int* __restrict__ in_len,
                                                         const int* __restrict__ tokens,
                                                         const int* __restrict__ out_len,
                                                         const int* __restrict__ count, const int* __restrict__ ref,
                                                         const int* __restrict__ ref_len, MwDims d,
                                                         MwPriorOf<Prior> prior, float* ws,
                                                         int* __restrict__ errors) {
  if (blockIdx.z == 2) {
    mwer_pair(tokens, out_len, count, ref, ref_len, d, prior, ws, errors);
  } else if (threadIdx.x < 64) {
    mwer_alpha_beta(heads, in_len, tokens, out_len, count, ref, ref_len, d, ws);
  }
}

// Workgroup i of four waves takes pairs 4 i + wave, then strides by the grid, lane n holding
// slot n (M <= 33): the posterior over the valid slots, the centred errors, the gradient weights
// w_n (without dloss), risk and loss_b.  A NaN likelihood counts as valid, so that it reaches
// the loss instead of dropping its entry.  The reference slot is valid iff it fits and no entry
// of the list has error count 0 (the reference is not in the list already).  With one workgroup
// (P <= MW_CLIPS_ONE_GROUP) wave j then sums loss_b of heads j, j + 4 in index order; a larger
// batch gets mwer_loss_sum_kernel as one more launch.
__device__ __forceinline__ void mwer_loss_sum(const float* lossb, int B, int lane, float* loss) {
  float acc = 0.0f;
  for (int b = lane; b < B; b += 64) acc += lossb[b];
  acc = wave_sum(acc);
  if (lane == 0) loss[0] = acc / (float)B;
}

__global__ __launch_bounds__(256) void mwer_clip_kernel(const int* __restrict__ count,
                                                        const int* __restrict__ errors, MwDims d,
                                                        float posterior_scale, float* ws,
                                                        float* __restrict__ loglik, float* __restrict__ posterior,
                                                        int* __restrict__ ref_valid, float* __restrict__ risk,
                                                        float* __restrict__ loss) {
  MwWs w(ws, d);
  const int lane = threadIdx.x & 63;
  for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < d.P; p += 4 * gridDim.x) {
    const int cnt = clampi(count[p], 0, d.N);
    const long e = (long)p * d.M + lane;
    const bool is_ref = d.with_ref && lane == d.N;
    const bool slot = lane < cnt || is_ref;
    const float ll = slot ? w.ll[e] : NEG_INF;
    const int en = lane < cnt ? errors[e] : 0;
    bool valid = ll != NEG_INF;
    int rv = 0;
    if (d.with_ref) {  // uniform
      const bool dup = __ballot(lane < cnt && en == 0) != 0ull;
      valid = valid && !(is_ref && dup);
      rv = __ballot(is_ref && valid) != 0ull;
    }
    if (ref_valid && lane == 0) ref_valid[p] = rv;
    const float tot = d.prior && slot ? ll + w.lmterm[e] : ll;
    const float z = valid ? posterior_scale * tot : NEG_INF;
    const float m = wave_max(z);
    const float ev = valid ? expf(z - m) : 0.0f;
    const float sum = wave_sum(ev);
    const float nv = wave_sum(valid ? 1.0f : 0.0f);
    const float err = valid ? (float)en : 0.0f;
    const float ebar = nv > 0.0f ? wave_sum(err) / nv : 0.0f;
    const float post = valid ? ev / sum : 0.0f;
    const float dn = valid ? err - ebar : 0.0f;
    const float rk = wave_sum(post * err);
    const float lb = wave_sum(post * dn);
    if (lane < d.M) {
      loglik[e] = ll;
      posterior[e] = post;
      w.w[e] = nv > 1.0f ? posterior_scale * post * (dn - lb) / (float)d.B : 0.0f;
    }
    if (lane == 0) {
      risk[p] = rk;
      w.lossb[p] = lb;
    }
  }
  if (gridDim.x > 1) return;  // uniform
  __syncthreads();
  for (int g = threadIdx.x >> 6; g * d.B < d.P; g += 4) mwer_loss_sum(w.lossb + (long)g * d.B, d.B, lane, loss + g);
}

// grid (G): the loss of head g
__global__ __launch_bounds__(64) void mwer_loss_sum_kernel(MwDims d, const float* ws, float* __restrict__ loss) {
  MwWs w(const_cast<float*>(ws), d);
  mwer_loss_sum(w.lossb + (long)blockIdx.x * d.B, d.B, threadIdx.x, loss + blockIdx.x);
}

// grid (T, P), one workgroup per logits row: g[c] = sum_n dloss w_n occ_n(t, c), n ascending, the
// reference slot last; every class of one slot is added by exactly one thread (the blank by
// thread 0, a label by the thread of its first occurrence, which sums the later ones in order).
// Then the CTC loss's row tail (ctc_grad_row_tail, ctc.h): the clamp gate, the row sum, the
// log-softmax backward.  dloss holds one float per head.
__global__ __launch_bounds__(MW_GRAD_THREADS) void mwer_grad_kernel(CtcHeads heads, const int* __restrict__ in_len,
                                                                    const int* __restrict__ tokens,
                                                                    const int* __restrict__ out_len,
                                                                    const int* __restrict__ count,
                                                                    const int* __restrict__ ref,
                                                                    const int* __restrict__ ref_len, MwDims d,
                                                                    const float* ws, const float* __restrict__ dloss,
                                                                    MwGrads grads) {
  __shared__ float ab[MW_MAX_L];
  __shared__ int tok_s[SCA_WER_MAX_LEN];
  __shared__ float g_s[SCA_CTC_MAX_C];
  __shared__ float red[4];
  MwWs w(const_cast<float*>(ws), d);
  const int p = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int g = p / d.B, b = p - g * d.B;
  const long hrow = (long)b * d.T + t;  // the row within head g's tensors
  const long row = (long)p * d.T + t;
  const float* xr = ctc_head(heads, g) + hrow * d.C;
  float* dr = mw_grad_head(grads, g) + hrow * d.C;
  const int cnt = clampi(count[p], 0, d.N);
  const int Tb = clampi(in_len[b], 0, d.T);
  const float gl = dloss[g];
  const int slots = cnt + d.with_ref;  // the list's entries, then the reference slot
  bool any = false;
  for (int k = 0; k < slots; ++k) any |= w.w[(long)p * d.M + (k < cnt ? k : d.N)] * gl != 0.0f;
  if (t >= Tb || !any) {  // uniform: frames past the input length, clips without a gradient
    for (int c = tid; c < d.C; c += MW_GRAD_THREADS) dr[c] = 0.0f;
    return;
  }
  const float m = w.rowstat[2 * row], ls = w.rowstat[2 * row + 1];
  for (int c = tid; c < d.C; c += MW_GRAD_THREADS) g_s[c] = 0.0f;
  const float lp0 = ctc_lp(ctc_lp_raw(xr[0], m, ls));
  for (int k = 0; k < slots; ++k) {
    const int n = k < cnt ? k : d.N;
    const long e = (long)p * d.M + n;
    const float wn = w.w[e] * gl;
    if (wn == 0.0f) continue;  // uniform
    const MwSlot slot = mw_slot(tokens, out_len, ref, ref_len, d, p, b, n);
    const int len = slot.len, L = 2 * len + 1;
    const float ll = w.ll[e];
    const float* al = w.alpha + (e * d.T + t) * w.Lm;
    const float* be = w.beta + (e * d.T + t) * w.Lm;
    __syncthreads();  // the previous slot's readers of ab, tok_s are done; g_s is zeroed
    for (int s = tid; s < L; s += MW_GRAD_THREADS) ab[s] = (al[s] + be[s]) - ll;
    for (int j = tid; j < len; j += MW_GRAD_THREADS) tok_s[j] = clampi(slot.tok[j], 0, d.C - 1);
    __syncthreads();
    if (tid < 64) {  // wave 0: the blank (every even state, plus odd states whose label is 0)
      float acc = 0.0f;
      for (int s = tid; s < L; s += 64)
        if (!(s & 1) || tok_s[s >> 1] == 0) acc += __expf(ab[s] - lp0);
      acc = wave_sum(acc);
      if (tid == 0) g_s[0] += wn * acc;
    } else {  // other waves: one thread per distinct non-blank label (its first occurrence)
      for (int j = tid - 64; j < len; j += MW_GRAD_THREADS - 64) {
        const int c = tok_s[j];
        bool first = c != 0;
        for (int i = 0; i < j && first; ++i) first = tok_s[i] != c;
        if (!first) continue;
        const float lpc = ctc_lp(ctc_lp_raw(xr[c], m, ls));
        float acc = 0.0f;
        for (int i = j; i < len; ++i)
          if (tok_s[i] == c) acc += __expf(ab[2 * i + 1] - lpc);
        g_s[c] += wn * acc;
      }
    }
  }
  __syncthreads();
  ctc_grad_row_tail<MW_GRAD_THREADS>(xr, dr, d.C, m, ls, g_s, red, tid, [&](int c, float) { return g_s[c]; });
}

bool mwer_dims_ok(int G, int B, int N, int T, int C, int H, int R) {
  return G >= 1 && G <= SCA_EVAL_MAX_HEADS && B >= 1 && (long)G * B <= 65535 && T >= 1 && C >= 1 &&
         C <= SCA_CTC_MAX_C && N >= 1 && N <= SCA_CTC_MAX_BEAM && H >= 1 && H <= SCA_WER_MAX_LEN && R >= 1 &&
         R <= SCA_WER_MAX_LEN;
}

#define MWER_LIMITS "bad arguments (1 <= B <= 65535, T >= 1, C <= 8192, 1 <= N <= 32, 1 <= H, R <= 128)"
#define MWER_NGRAM_LIMITS \
  "; with a model: order in 1..3, C the logits', counts >= 0, the arrays of the orders in use"
#define MWER_HEADS_LIMITS \
  "bad arguments (1 <= G <= 8, B >= 1, G B <= 65535, T >= 1, C <= 8192, 1 <= N <= 32, 1 <= H, R <= 128, finite weights)"

// One call of any of the four entry points, forward or backward.  A single-tensor entry point is
// G = 1 with its tensor in heads->logits[0] (and dlogits->dlogits[0]), with_ref = 0, no prior and
// ref_valid = NULL; its backward has no references (R = 1).  A backward is initialised up to
// dlogits and leaves the forward's fields 0 / NULL; a forward has dloss = dlogits = NULL.
struct MwCall {
  const char* name;  // of the entry point, for the errors
  bool grouped;      // the _heads form: its limits, ref_valid required, the references in the backward too
  const sca_decode_heads* heads;
  int G;
  const int *in_len, *tokens, *out_len, *count, *ref, *ref_len;
  int B, N, T, C, H, R, with_ref;
  const float* ws;     // the forward writes it
  const float* dloss;  // backward
  const sca_mwer_grads* dlogits;
  MwPrior prior;  // forward
  const sca_ngram_lm* ngram;  // forward, the _ngram entry point: the trie in place of prior.lm (NULL: none)
  bool sparse;                // the _ngram entry point
  float posterior_scale;
  float *loglik, *posterior;
  int *errors, *ref_valid;
  float *risk, *loss;
};

bool mw_call_ok(const MwCall& c, bool bwd) {
  bool ok = c.heads && mwer_dims_ok(c.G, c.B, c.N, c.T, c.C, c.H, c.R) && c.in_len && c.tokens && c.out_len &&
            c.count && c.ws && ((c.ref && c.ref_len) || (bwd && !c.grouped));
  if (bwd) {
    ok = ok && c.dloss && c.dlogits;
  } else {
    ok = ok && c.prior.weight - c.prior.weight == 0.0f && c.prior.bonus - c.prior.bonus == 0.0f &&
         c.posterior_scale == c.posterior_scale && c.loglik && c.posterior && c.errors &&
         (c.ref_valid || !c.grouped) && c.risk && c.loss;
  }
  for (int g = 0; ok && g < c.G; ++g) ok = c.heads->logits[g] && (!bwd || c.dlogits->dlogits[g]);
  if (ok && !bwd && c.sparse) ok = ctc_ngram_ok(c.ngram) && (!c.ngram || c.ngram->C == c.C);
  if (!ok) {
    char msg[384];
    snprintf(msg, sizeof(msg), "%s: %s%s", c.name, c.grouped ? MWER_HEADS_LIMITS : MWER_LIMITS,
             c.sparse ? MWER_NGRAM_LIMITS : "");
    sca_set_error(msg);
  }
  return ok;
}

// The forward of every entry point: three launches, four above MW_CLIPS_ONE_GROUP pairs.  The
// prior's term is computed only where it can differ from 0: with a table or a length bonus.
int mwer_fwd(const MwCall& c, void* stream) {
  if (!mw_call_ok(c, false)) return SCA_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const MwDims d = mw_dims(c.G, c.B, c.N, c.T, c.C, c.H, c.R, c.with_ref,
                           c.prior.lm || c.ngram || c.prior.bonus != 0.0f);
  float* ws = const_cast<float*>(c.ws);
  if (c.G == 1) {
    sca_ctc_rowstat_launch(c.heads->logits[0], ws, (long)d.B * d.T, d.C, st);
  } else {
    sca_ctc_rowstat_heads_launch(c.heads, c.G, ws, (long)d.B * d.T, d.C, st);
  }
  if (c.sparse) {
    hipLaunchKernelGGL(mwer_entry_kernel<CtcNgramPrior>, dim3(d.M, d.P, 3), dim3(128), 0, st,
                       ctc_heads_of(c.heads, c.G), c.in_len, c.tokens, c.out_len, c.count, c.ref, c.ref_len, d,
                       MwPriorOf<CtcNgramPrior>{{ctc_ngram_of(c.ngram)}, c.prior.weight, c.prior.bonus}, ws, c.errors);
  } else {
    hipLaunchKernelGGL(mwer_entry_kernel<CtcBigramPrior>, dim3(d.M, d.P, 3), dim3(128), 0, st,
                       ctc_heads_of(c.heads, c.G), c.in_len, c.tokens, c.out_len, c.count, c.ref, c.ref_len, d,
                       MwPriorOf<CtcBigramPrior>{{c.prior.lm, d.C}, c.prior.weight, c.prior.bonus}, ws, c.errors);
  }
  const int groups = d.P <= MW_CLIPS_ONE_GROUP ? 1 : (d.P + 3) / 4;
  hipLaunchKernelGGL(mwer_clip_kernel, dim3(groups), dim3(256), 0, st, c.count, c.errors, d, c.posterior_scale, ws,
                     c.loglik, c.posterior, c.ref_valid, c.risk, c.loss);
  if (groups > 1) hipLaunchKernelGGL(mwer_loss_sum_kernel, dim3(c.G), dim3(64), 0, st, d, c.ws, c.loss);
  return sca_launch_status(c.name);
}

// The backward of every entry point: one launch.  The prior does not reach the gradient.
int mwer_bwd(const MwCall& c, void* stream) {
  if (!mw_call_ok(c, true)) return SCA_ERR_ARG;
  MwGrads grads = {};
  for (int g = 0; g < SCA_EVAL_MAX_HEADS; ++g) grads.dx[g] = c.dlogits->dlogits[g < c.G ? g : 0];
  const MwDims d = mw_dims(c.G, c.B, c.N, c.T, c.C, c.H, c.R, c.with_ref, 0);
  hipLaunchKernelGGL(mwer_grad_kernel, dim3(d.T, d.P), dim3(MW_GRAD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     ctc_heads_of(c.heads, c.G), c.in_len, c.tokens, c.out_len, c.count, c.ref, c.ref_len, d, c.ws,
                     c.dloss, grads);
  return sca_launch_status(c.name);
}

}  // namespace

extern "C" long sca_mwer_workspace_floats(int B, int N, int T, int H) {
  if (B < 1 || N < 1 || T < 1 || H < 1) return 0;
  return mw_ws_floats(B, N, T, H, false);
}

extern "C" long sca_mwer_heads_workspace_floats(int G, int B, int N, int T, int H, int R, int with_ref) {
  if (G < 1 || B < 1 || N < 1 || T < 1 || H < 1 || R < 1) return 0;
  return mw_ws_floats((long)G * B, N + (with_ref ? 1 : 0), T, with_ref && R > H ? R : H, true);
}

extern "C" int sca_mwer_fwd(const float* logits, const int* in_len, const int* tokens, const int* out_len,
                            const int* count, const int* ref, const int* ref_len, int B, int N, int T, int C, int H,
                            int R, float posterior_scale, float* loglik, float* posterior, int* errors, float* risk,
                            float* loss, float* ws, void* stream) {
  const sca_decode_heads one = {{logits}};
  return mwer_fwd({"sca_mwer_fwd", false, &one, 1, in_len, tokens, out_len, count, ref, ref_len, B, N, T, C, H, R, 0,
                   ws, nullptr, nullptr, {}, nullptr, false, posterior_scale, loglik, posterior, errors, nullptr, risk,
                   loss},
                  stream);
}

extern "C" int sca_mwer_bwd(const float* logits, const int* in_len, const int* tokens, const int* out_len,
                            const int* count, int B, int N, int T, int C, int H, const float* dloss, const float* ws,
                            float* dlogits, void* stream) {
  const sca_decode_heads one = {{logits}};
  const sca_mwer_grads grads = {{dlogits}};
  return mwer_bwd({"sca_mwer_bwd", false, &one, 1, in_len, tokens, out_len, count, nullptr, nullptr, B, N, T, C, H, 1,
                   0, ws, dloss, &grads},
                  stream);
}

extern "C" int sca_mwer_heads_fwd(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                                  const int* out_len, const int* count, const int* ref, const int* ref_len, int B,
                                  int N, int T, int C, int H, int R, int with_ref, const float* lm, float lm_weight,
                                  float length_bonus, float posterior_scale, float* loglik, float* posterior,
                                  int* errors, int* ref_valid, float* risk, float* loss, float* ws, void* stream) {
  return mwer_fwd({"sca_mwer_heads_fwd", true, heads, G, in_len, tokens, out_len, count, ref, ref_len, B, N, T, C, H, R,
                   with_ref, ws, nullptr, nullptr, {lm, lm_weight, length_bonus}, nullptr, false, posterior_scale,
                   loglik, posterior, errors, ref_valid, risk, loss},
                  stream);
}

extern "C" int sca_mwer_heads_fwd_ngram(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                                        const int* out_len, const int* count, const int* ref, const int* ref_len,
                                        int B, int N, int T, int C, int H, int R, int with_ref,
                                        const sca_ngram_lm* lm, float lm_weight, float length_bonus,
                                        float posterior_scale, float* loglik, float* posterior, int* errors,
                                        int* ref_valid, float* risk, float* loss, float* ws, void* stream) {
  return mwer_fwd({"sca_mwer_heads_fwd_ngram", true, heads, G, in_len, tokens, out_len, count, ref, ref_len, B, N, T,
                   C, H, R, with_ref, ws, nullptr, nullptr, {nullptr, lm_weight, length_bonus}, lm, true,
                   posterior_scale, loglik, posterior, errors, ref_valid, risk, loss},
                  stream);
}

extern "C" int sca_mwer_heads_bwd(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                                  const int* out_len, const int* count, const int* ref, const int* ref_len, int B,
                                  int N, int T, int C, int H, int R, int with_ref, const float* dloss, const float* ws,
                                  const sca_mwer_grads* dlogits, void* stream) {
  return mwer_bwd({"sca_mwer_heads_bwd", true, heads, G, in_len, tokens, out_len, count, ref, ref_len, B, N, T, C, H, R,
                   with_ref, ws, dloss, dlogits},
                  stream);
}
