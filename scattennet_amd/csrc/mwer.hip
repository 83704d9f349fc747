// Minimum word error rate (MWER) training loss over an n-best list (include/scatten.h): the
// expected number of errors of the list's hypotheses under the model's own posterior over the
// list, with exact CTC likelihoods, and its gradient with respect to the logits.  The reference
// has none of this.
//   fwd: row statistics (the pass the CTC loss and the decoders share) -> one launch with alpha
//        and beta of every (clip, entry), one wave64 each, beside its error count, the alignment
//        of wer_pair.h -> posterior, centred errors, gradient weights, risk, loss
//   bwd: one workgroup per (clip, frame): sum_n w_n occ_n(t, .) in one LDS row, n ascending,
//        then the clamp gate and the log-softmax backward: ONE dense pass for the N hypotheses
// No float atomics; every sum over entries, states and clips runs in a fixed order, so the
// results are deterministic and a replayed capture is bitwise the eager call.
#include "ctc.h"
#include "wer_pair.h"

namespace {

constexpr int MW_MAX_L = 2 * SCA_WER_MAX_LEN + 1;  // states of the longest hypothesis
constexpr int MW_K = (MW_MAX_L + 63) / 64;         // states per lane of the recursion's wave
constexpr int MW_PAD = 2;                          // -inf cells either side of an LDS state row
constexpr int MW_GRAD_THREADS = 256;
constexpr int MW_CLIPS_ONE_GROUP = 64;  // batches up to this size: per-clip statistics and the loss in one workgroup

struct MwDims {
  int B, N, T, C, H, R;
};

// workspace layout (floats): rowstat[B T 2] | alpha[B N T Lm] | beta[B N T Lm] | ll[B N] |
// w[B N] | lossb[B], Lm = 2 H + 1
struct MwWs {
  float *rowstat, *alpha, *beta, *ll, *w, *lossb;
  long Lm;
  __host__ __device__ MwWs(float* ws, MwDims d) {
    const long BT = (long)d.B * d.T, BN = (long)d.B * d.N;
    Lm = 2L * d.H + 1;
    rowstat = ws;
    alpha = rowstat + 2 * BT;
    beta = alpha + BN * d.T * Lm;
    ll = beta + BN * d.T * Lm;
    w = ll + BN;
    lossb = w + BN;
  }
};

// One wave64 per (entry, clip, direction) of mwer_entry_kernel: z = 0 the alpha recursion over
// the frames [0, in_len), z = 1 the beta one.  Lane l holds states l, l + 64, ..; a frame's row
// goes through a wave-private LDS row for the neighbours s -+ 1, s -+ 2, so a frame costs no
// workgroup barrier.  The emissions lp[t, label(s)] do not depend on the recursion: the next
// frame's gathers are issued before this frame's row is computed.
__device__ __forceinline__ void mwer_alpha_beta(const float* __restrict__ x, const int* __restrict__ in_len,
                                                const int* __restrict__ tokens, const int* __restrict__ out_len,
                                                const int* __restrict__ count, MwDims d, float* ws) {
  __shared__ float buf[2][MW_MAX_L + 2 * MW_PAD];
  MwWs w(ws, d);
  const int n = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const bool beta_pass = blockIdx.z == 1;
  const long e = (long)b * d.N + n;
  const int cnt = clampi(count[b], 0, d.N);
  const int Tb = clampi(in_len[b], 0, d.T);
  if (n >= cnt) {  // uniform: entries past count are ignored
    if (!beta_pass && lane == 0) w.ll[e] = NEG_INF;
    return;
  }
  const int len = clampi(out_len[e], 0, d.H);
  if (Tb == 0) {  // no frame: only the empty hypothesis fits, with likelihood 1
    if (!beta_pass && lane == 0) w.ll[e] = len == 0 ? 0.0f : NEG_INF;
    return;
  }
  const int L = 2 * len + 1;
  const int* tok = tokens + e * d.H;
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
  const float* xb = x + (long)b * d.T * d.C;
  const float* rs = w.rowstat + 2L * b * d.T;
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

// z = 2 of mwer_entry_kernel, one workgroup per (entry, clip): errors[b, n] = num_del + num_ins +
// num_sub of reference b against entry n; 0 for the entries past count
__device__ __forceinline__ void mwer_pair(const int* __restrict__ tokens, const int* __restrict__ out_len,
                                          const int* __restrict__ count, const int* __restrict__ ref,
                                          const int* __restrict__ ref_len, MwDims d, int* __restrict__ errors) {
  __shared__ int c4[4];
  const int n = blockIdx.x, b = blockIdx.y;
  const long e = (long)b * d.N + n;
  if (n >= clampi(count[b], 0, d.N)) {  // uniform over the workgroup
    if (threadIdx.x == 0) errors[e] = 0;
    return;
  }
  const int R = clampi(ref_len[b], 0, d.R), H = clampi(out_len[e], 0, d.H);
  wer_pair(ref + (long)b * d.R, R, tokens + e * d.H, H, c4);
  if (threadIdx.x == 0) errors[e] = c4[0] + c4[1] + c4[2];  // thread 0 wrote c4
}

// grid (N, B, 3), 128 threads: the three independent jobs of one (entry, clip) in ONE launch, so
// that the alignment (an anti-diagonal sweep and a serial back-trace) runs beside the two
// recursions instead of after them.  z = 0, 1: wave 0 runs the recursion, wave 1 leaves at once
// (the recursion uses no workgroup barrier); z = 2: both waves run wer_pair.
__global__ __launch_bounds__(128) void mwer_entry_kernel(const float* __restrict__ x, const int* __restrict__ in_len,
                                                         const int* __restrict__ tokens,
                                                         const int* __restrict__ out_len,
                                                         const int* __restrict__ count, const int* __restrict__ ref,
                                                         const int* __restrict__ ref_len, MwDims d, float* ws,
                                                         int* __restrict__ errors) {
  if (blockIdx.z == 2) {
    mwer_pair(tokens, out_len, count, ref, ref_len, d, errors);
  } else if (threadIdx.x < 64) {
    mwer_alpha_beta(x, in_len, tokens, out_len, count, d, ws);
  }
}

// Workgroup g of four waves takes clips 4 g + wave, then strides by the grid, lane n holding
// entry n: the posterior over the valid entries, the centred errors, the gradient weights w_n
// (without dloss), risk and loss_b.  A NaN likelihood counts as valid, so that it reaches the
// loss instead of dropping its entry.  With one workgroup (B <= MW_CLIPS_ONE_GROUP) wave 0 then
// sums loss_b in index order; a larger batch gets mwer_loss_sum_kernel as one more launch.
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
                                                        float* __restrict__ risk, float* __restrict__ loss) {
  MwWs w(ws, d);
  const int lane = threadIdx.x & 63;
  for (int b = blockIdx.x * 4 + (threadIdx.x >> 6); b < d.B; b += 4 * gridDim.x) {
    const int cnt = clampi(count[b], 0, d.N);
    const long e = (long)b * d.N + lane;
    const float ll = lane < cnt ? w.ll[e] : NEG_INF;
    const bool valid = ll != NEG_INF;
    const float z = valid ? posterior_scale * ll : NEG_INF;
    const float m = wave_max(z);
    const float ev = valid ? expf(z - m) : 0.0f;
    const float sum = wave_sum(ev);
    const float nv = wave_sum(valid ? 1.0f : 0.0f);
    const float err = valid ? (float)errors[e] : 0.0f;
    const float ebar = nv > 0.0f ? wave_sum(err) / nv : 0.0f;
    const float post = valid ? ev / sum : 0.0f;
    const float dn = valid ? err - ebar : 0.0f;
    const float rk = wave_sum(post * err);
    const float lb = wave_sum(post * dn);
    if (lane < d.N) {
      loglik[e] = ll;
      posterior[e] = post;
      w.w[e] = nv > 1.0f ? posterior_scale * post * (dn - lb) / (float)d.B : 0.0f;
    }
    if (lane == 0) {
      risk[b] = rk;
      w.lossb[b] = lb;
    }
  }
  if (gridDim.x > 1) return;  // uniform
  __syncthreads();
  if (threadIdx.x < 64) mwer_loss_sum(w.lossb, d.B, lane, loss);
}

__global__ __launch_bounds__(64) void mwer_loss_sum_kernel(MwDims d, const float* ws, float* __restrict__ loss) {
  MwWs w(const_cast<float*>(ws), d);
  mwer_loss_sum(w.lossb, d.B, threadIdx.x, loss);
}

// grid (T, B), one workgroup per logits row: g[c] = sum_n dloss w_n occ_n(t, c), n ascending;
// every class of one entry is added by exactly one thread (the blank by thread 0, a label by
// the thread of its first occurrence, which sums the later ones in order).  Then the CTC
// loss's row tail (ctc_grad_row_tail, ctc.h): the clamp gate, the row sum, the log-softmax backward.
__global__ __launch_bounds__(MW_GRAD_THREADS) void mwer_grad_kernel(const float* __restrict__ x,
                                                                    const int* __restrict__ in_len,
                                                                    const int* __restrict__ tokens,
                                                                    const int* __restrict__ out_len,
                                                                    const int* __restrict__ count, MwDims d,
                                                                    const float* ws, const float* __restrict__ dloss,
                                                                    float* __restrict__ dx) {
  __shared__ float ab[MW_MAX_L];
  __shared__ int tok_s[SCA_WER_MAX_LEN];
  __shared__ float g_s[SCA_CTC_MAX_C];
  __shared__ float red[4];
  MwWs w(const_cast<float*>(ws), d);
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const long row = (long)b * d.T + t;
  const float* xr = x + row * d.C;
  float* dr = dx + row * d.C;
  const int cnt = clampi(count[b], 0, d.N);
  const int Tb = clampi(in_len[b], 0, d.T);
  const float gl = dloss[0];
  bool any = false;
  for (int n = 0; n < cnt; ++n) any |= w.w[(long)b * d.N + n] * gl != 0.0f;
  if (t >= Tb || !any) {  // uniform: frames past the input length, clips without a gradient
    for (int c = tid; c < d.C; c += MW_GRAD_THREADS) dr[c] = 0.0f;
    return;
  }
  const float m = w.rowstat[2 * row], ls = w.rowstat[2 * row + 1];
  for (int c = tid; c < d.C; c += MW_GRAD_THREADS) g_s[c] = 0.0f;
  const float lp0 = ctc_lp(ctc_lp_raw(xr[0], m, ls));
  for (int n = 0; n < cnt; ++n) {
    const long e = (long)b * d.N + n;
    const float wn = w.w[e] * gl;
    if (wn == 0.0f) continue;  // uniform
    const int len = clampi(out_len[e], 0, d.H), L = 2 * len + 1;
    const float ll = w.ll[e];
    const float* al = w.alpha + (e * d.T + t) * w.Lm;
    const float* be = w.beta + (e * d.T + t) * w.Lm;
    __syncthreads();  // the previous entry's readers of ab, tok_s are done; g_s is zeroed
    for (int s = tid; s < L; s += MW_GRAD_THREADS) ab[s] = (al[s] + be[s]) - ll;
    for (int j = tid; j < len; j += MW_GRAD_THREADS) tok_s[j] = clampi(tokens[e * d.H + j], 0, d.C - 1);
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
        for (int k = 0; k < j && first; ++k) first = tok_s[k] != c;
        if (!first) continue;
        const float lpc = ctc_lp(ctc_lp_raw(xr[c], m, ls));
        float acc = 0.0f;
        for (int k = j; k < len; ++k)
          if (tok_s[k] == c) acc += __expf(ab[2 * k + 1] - lpc);
        g_s[c] += wn * acc;
      }
    }
  }
  __syncthreads();
  ctc_grad_row_tail<MW_GRAD_THREADS>(xr, dr, d.C, m, ls, g_s, red, tid, [&](int c, float) { return g_s[c]; });
}

bool mwer_dims_ok(int B, int N, int T, int C, int H, int R) {
  return B >= 1 && B <= 65535 && T >= 1 && C >= 1 && C <= SCA_CTC_MAX_C && N >= 1 && N <= SCA_CTC_MAX_BEAM &&
         H >= 1 && H <= SCA_WER_MAX_LEN && R >= 1 && R <= SCA_WER_MAX_LEN;
}

#define MWER_LIMITS "bad arguments (1 <= B <= 65535, T >= 1, C <= 8192, 1 <= N <= 32, 1 <= H, R <= 128)"

}  // namespace

extern "C" long sca_mwer_workspace_floats(int B, int N, int T, int H) {
  if (B < 1 || N < 1 || T < 1 || H < 1) return 0;
  const long BT = (long)B * T, BN = (long)B * N;
  return 2 * BT + 2 * BN * T * (2L * H + 1) + 2 * BN + B;
}

extern "C" int sca_mwer_fwd(const float* logits, const int* in_len, const int* tokens, const int* out_len,
                            const int* count, const int* ref, const int* ref_len, int B, int N, int T, int C, int H,
                            int R, float posterior_scale, float* loglik, float* posterior, int* errors, float* risk,
                            float* loss, float* ws, void* stream) {
  if (!mwer_dims_ok(B, N, T, C, H, R) || !logits || !in_len || !tokens || !out_len || !count || !ref || !ref_len ||
      !(posterior_scale == posterior_scale) || !loglik || !posterior || !errors || !risk || !loss || !ws) {
    sca_set_error("sca_mwer_fwd: " MWER_LIMITS);
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const MwDims d{B, N, T, C, H, R};
  sca_ctc_rowstat_launch(logits, ws, (long)B * T, C, st);
  hipLaunchKernelGGL(mwer_entry_kernel, dim3(N, B, 3), dim3(128), 0, st, logits, in_len, tokens, out_len, count, ref,
                     ref_len, d, ws, errors);
  const int groups = B <= MW_CLIPS_ONE_GROUP ? 1 : (B + 3) / 4;
  hipLaunchKernelGGL(mwer_clip_kernel, dim3(groups), dim3(256), 0, st, count, errors, d, posterior_scale, ws, loglik,
                     posterior, risk, loss);
  if (groups > 1) hipLaunchKernelGGL(mwer_loss_sum_kernel, dim3(1), dim3(64), 0, st, d, ws, loss);
  return sca_launch_status("sca_mwer_fwd");
}

extern "C" int sca_mwer_bwd(const float* logits, const int* in_len, const int* tokens, const int* out_len,
                            const int* count, int B, int N, int T, int C, int H, const float* dloss, const float* ws,
                            float* dlogits, void* stream) {
  if (!mwer_dims_ok(B, N, T, C, H, 1) || !logits || !in_len || !tokens || !out_len || !count || !dloss || !ws ||
      !dlogits) {
    sca_set_error("sca_mwer_bwd: " MWER_LIMITS);
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(mwer_grad_kernel, dim3(T, B), dim3(MW_GRAD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     logits, in_len, tokens, out_len, count, MwDims{B, N, T, C, H, 1}, ws, dloss, dlogits);
  return sca_launch_status("sca_mwer_bwd");
}
