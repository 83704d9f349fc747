// Recognition-head losses of MSCA_Net:
//   * CTC: MSCA_Net.compute_loss (model/__init__.py:241-290) = log_softmax -> clamp(-100, 0)
//     -> nn.CTCLoss(blank=0, reduction='none', zero_infinity=True) -> mean over finite
//     losses -> clamp(0, 100).  The log-space alpha/beta recursions and the gradient follow
//     torch's published CPU algorithm (aten/src/ATen/native/LossCTC.cpp, the third-party op
//     the reference calls; formulas restated in oracle/heads_oracle.py).
//   * SeqKD (loss.py:5-21) with the weight and clamp(-100, 100) of model/__init__.py:203-214.
//   * clamp(+-50) of RecognitionHead.forward (model/__init__.py:54-58) with its gradient gate.
// All of it is latency-bound (one sample's alpha row depends on the previous frame's); the
// HBM traffic is a few (B, T, C) passes.  Batch-major logits (B, T, C): the reference's
// permute(1, 0, 2) (:245) is a view and never materialised.
#include "ctc.h"
#include "seqkd.h"

namespace {

constexpr int CTC_THREADS = 256;
constexpr int CTC_MAX_L = 2 * SCA_CTC_MAX_S + 1;

struct CtcDims {
  int B, T, C, S;
};

// workspace layout (floats): rowstat[B*T*2] | alpha[B*T*Lm] | beta[B*T*Lm] | nll[B] | scale[B]
struct CtcWs {
  float *rowstat, *alpha, *beta, *nll, *scale;
  __host__ __device__ CtcWs(float* ws, CtcDims d) {
    const long Lm = 2L * d.S + 1, BT = (long)d.B * d.T;
    rowstat = ws;
    alpha = rowstat + 2 * BT;
    beta = alpha + BT * Lm;
    nll = beta + BT * Lm;
    scale = nll + d.B;
  }
};

__device__ __forceinline__ void ctc_lengths(const int* in_len, const int* tgt_len, int b, CtcDims d, int& Tb,
                                            int& Sb) {
  // model/__init__.py:262-266: clamp both to >= 1, then input = max(input, target)
  Sb = max(tgt_len[b], 1);
  Tb = max(max(in_len[b], 1), Sb);
  Sb = min(Sb, d.S);  // host validates; the clamps only keep a bad call in bounds
  Tb = min(Tb, d.T);
}

__device__ __forceinline__ int ctc_label(const int* lab, int s, int C) {
  if (!(s & 1)) return 0;
  return clampi(lab[(s - 1) >> 1], 0, C - 1);
}

// one wave per (b, t) row: max and log-sum-exp of the logits row
__global__ __launch_bounds__(256) void ctc_rowstat_kernel(const float* __restrict__ x, float* __restrict__ rowstat,
                                                          long rows, int C) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  ctc_row_stat(x + row * C, C, lane, rowstat + 2 * row);
}

// grid (B, 2): y = 0 runs the alpha (forward) recursion, y = 1 the beta (backward) one
__global__ __launch_bounds__(CTC_THREADS) void ctc_alpha_beta_kernel(const float* __restrict__ x,
                                                                     const int* __restrict__ labels,
                                                                     const int* __restrict__ in_len,
                                                                     const int* __restrict__ tgt_len, CtcDims d,
                                                                     float* ws) {
  __shared__ float buf[2][CTC_MAX_L];
  __shared__ int lab_s[CTC_MAX_L];
  CtcWs w(ws, d);
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool beta_pass = blockIdx.y == 1;
  int Tb, Sb;
  ctc_lengths(in_len, tgt_len, b, d, Tb, Sb);
  const int L = 2 * Sb + 1;
  const long Lm = 2L * d.S + 1;
  const int* lab = labels + (long)b * d.S;
  for (int s = tid; s < L; s += CTC_THREADS) lab_s[s] = ctc_label(lab, s, d.C);
  __syncthreads();
  const float* xb = x + (long)b * d.T * d.C;
  const float* rs = w.rowstat + 2L * b * d.T;
  float* out = (beta_pass ? w.beta : w.alpha) + (long)b * d.T * Lm;
  auto lp_at = [&](int t, int s) {
    const float m = rs[2 * t], ls = rs[2 * t + 1];
    return ctc_lp(ctc_lp_raw(xb[(long)t * d.C + lab_s[s]], m, ls));
  };
  int cur = 0;
  // first frame (alpha: t = 0, beta: t = Tb - 1)
  const int t0 = beta_pass ? Tb - 1 : 0;
  for (int s = tid; s < L; s += CTC_THREADS) {
    float v = NEG_INF;
    if (!beta_pass && s < 2) v = lp_at(t0, s);
    if (beta_pass && s >= L - 2) v = lp_at(t0, s);
    buf[cur][s] = v;
    out[(long)t0 * Lm + s] = v;
  }
  __syncthreads();
  for (int step = 1; step < Tb; ++step) {
    const int t = beta_pass ? Tb - 1 - step : step;
    const float* prev = buf[cur];
    float* nxt = buf[cur ^ 1];
    for (int s = tid; s < L; s += CTC_THREADS) {
      const int l = lab_s[s];
      float a1 = prev[s], a2, a3;
      if (!beta_pass) {
        a2 = s > 0 ? prev[s - 1] : NEG_INF;
        a3 = (s > 1 && lab_s[s - 2] != l) ? prev[s - 2] : NEG_INF;
      } else {
        a2 = s < L - 1 ? prev[s + 1] : NEG_INF;
        a3 = (s < L - 2 && lab_s[s + 2] != l) ? prev[s + 2] : NEG_INF;
      }
      const float v = lse3(a1, a2, a3) + lp_at(t, s);
      nxt[s] = v;
      out[(long)t * Lm + s] = v;
    }
    cur ^= 1;
    __syncthreads();
  }
  if (!beta_pass && tid == 0) {
    // nll = -log(exp(alpha[Tb-1][L-1]) + exp(alpha[Tb-1][L-2])); zero_infinity
    w.nll[b] = -ctc_end_loglik(buf[cur][L - 1], buf[cur][L - 2]);  // +inf kept: zero_infinity below
  }
}

// one workgroup: loss = clamp(mean(finite nll), 0, 100); per-sample d loss / d nll
__global__ __launch_bounds__(256) void ctc_finalize_kernel(CtcDims d, float* ws, float* nll_out, float* loss) {
  __shared__ float red_s[4], red_n[4];
  CtcWs w(ws, d);
  const int tid = threadIdx.x;
  float s = 0.0f, n = 0.0f;
  for (int b = tid; b < d.B; b += 256) {
    const float raw = w.nll[b];
    const float v = raw == __builtin_huge_valf() ? 0.0f : raw;  // zero_infinity=True
    if (isfinite(v)) { s += v; n += 1.0f; }
    if (nll_out) nll_out[b] = v;
  }
  s = wave_sum(s);
  n = wave_sum(n);
  if ((tid & 63) == 0) { red_s[tid >> 6] = s; red_n[tid >> 6] = n; }
  __syncthreads();
  const float S = red_s[0] + red_s[1] + red_s[2] + red_s[3];
  const float N = red_n[0] + red_n[1] + red_n[2] + red_n[3];
  // model/__init__.py:276-283: no finite loss -> 0 (no gradient); else clamp(mean, 0, 100)
  const float mean = N > 0.0f ? S / N : 0.0f;
  const float gate = (N > 0.0f && mean >= 0.0f && mean <= 100.0f) ? 1.0f / N : 0.0f;
  if (tid == 0) loss[0] = fminf(fmaxf(mean, 0.0f), 100.0f);
  // zero_infinity'd samples count in the mean with loss 0 but get no gradient
  for (int b = tid; b < d.B; b += 256) w.scale[b] = isfinite(w.nll[b]) ? gate : 0.0f;
}

// one workgroup per (b, t) row: d loss / d logits (through the CTC gradient, the log-prob
// clamp and log_softmax)
__global__ __launch_bounds__(CTC_THREADS) void ctc_grad_kernel(const float* __restrict__ x,
                                                               const int* __restrict__ labels,
                                                               const int* __restrict__ in_len,
                                                               const int* __restrict__ tgt_len, CtcDims d,
                                                               const float* ws, const float* __restrict__ dloss,
                                                               float* __restrict__ dx) {
  __shared__ float ab[CTC_MAX_L];
  __shared__ float g_s[SCA_CTC_MAX_C];
  __shared__ float red[4];
  CtcWs w(const_cast<float*>(ws), d);
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const long row = (long)b * d.T + t;
  const float* xr = x + row * d.C;
  float* dr = dx + row * d.C;
  int Tb, Sb;
  ctc_lengths(in_len, tgt_len, b, d, Tb, Sb);
  const float gr = dloss[0] * w.scale[b];
  if (t >= Tb || gr == 0.0f) {  // frames past the input length, zero_infinity samples, gated loss
    for (int c = tid; c < d.C; c += CTC_THREADS) dr[c] = 0.0f;
    return;
  }
  const int L = 2 * Sb + 1;
  const long Lm = 2L * d.S + 1;
  const int* lab = labels + (long)b * d.S;
  const float* al = w.alpha + row * Lm;
  const float* be = w.beta + row * Lm;
  for (int s = tid; s < L; s += CTC_THREADS) ab[s] = al[s] + be[s];
  for (int c = tid; c < d.C; c += CTC_THREADS) g_s[c] = NEG_INF;
  __syncthreads();
  // lcab[c] = logsumexp over states s with l'(s) = c of alpha + beta
  if (tid < 64) {  // wave 0: the blank (every even state, plus odd states whose label is 0)
    float m = NEG_INF;
    for (int s = tid; s < L; s += 64)
      if (!(s & 1) || ctc_label(lab, s, d.C) == 0) m = fmaxf(m, ab[s]);
    m = wave_max(m);
    float acc = 0.0f;
    if (m != NEG_INF)
      for (int s = tid; s < L; s += 64)
        if (!(s & 1) || ctc_label(lab, s, d.C) == 0) acc += __expf(ab[s] - m);
    acc = wave_sum(acc);
    if (tid == 0) g_s[0] = m == NEG_INF ? NEG_INF : __logf(acc) + m;
  } else {  // other waves: one thread per distinct non-blank label (its first occurrence)
    for (int j = tid - 64; j < Sb; j += CTC_THREADS - 64) {
      const int c = ctc_label(lab, 2 * j + 1, d.C);
      bool first = c != 0;
      for (int k = 0; k < j && first; ++k) first = ctc_label(lab, 2 * k + 1, d.C) != c;
      if (!first) continue;
      float m = NEG_INF;
      for (int k = j; k < Sb; ++k)
        if (ctc_label(lab, 2 * k + 1, d.C) == c) m = fmaxf(m, ab[2 * k + 1]);
      float acc = 0.0f;
      if (m != NEG_INF)
        for (int k = j; k < Sb; ++k)
          if (ctc_label(lab, 2 * k + 1, d.C) == c) acc += __expf(ab[2 * k + 1] - m);
      g_s[c] = m == NEG_INF ? NEG_INF : __logf(acc) + m;
    }
  }
  __syncthreads();
  const float m = w.rowstat[2 * row], ls = w.rowstat[2 * row + 1];
  const float nll = w.nll[b];
  ctc_grad_row_tail<CTC_THREADS>(xr, dr, d.C, m, ls, g_s, red, tid, [&](int c, float raw) {
    const float lp = ctc_lp(raw);
    // torch ctc_loss_backward: (exp(lp) - exp(lcab + nll - lp)) * grad_out
    return (__expf(lp) - __expf(g_s[c] + nll - lp)) * gr;
  });
}

// ------------------------------------------------------------------------------------ SeqKD
// The row arithmetic is seqkd.h's (shared with the grouped call of distill.hip).
template <bool VALID>
__global__ __launch_bounds__(256) void kd_row_kernel(KdArgs a, float* ws) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.R) return;
  kd_row<VALID>(a, ws, row, lane);
}

template <bool VALID>
__global__ __launch_bounds__(256) void kd_finalize_kernel(KdArgs a, float* ws, float* loss) {
  __shared__ float red[4];
  kd_finalize<VALID>(a, ws, loss, red, threadIdx.x);
}

template <bool VALID>
__global__ __launch_bounds__(256) void kd_grad_kernel(KdArgs a, const float* ws, const float* dloss, float* ds,
                                                      float* dq) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.R) return;
  kd_grad_row<VALID>(a, ws, dloss, ds, dq, row, lane);
}

__global__ __launch_bounds__(256) void clamp_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                    const float* __restrict__ dy, float* __restrict__ dx, long n,
                                                    float lo, float hi) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = x[i];
    if (dy) dx[i] = (v >= lo && v <= hi) ? dy[i] : 0.0f;  // torch clamp backward gate
    else y[i] = v < lo ? lo : (v > hi ? hi : v);  // a NaN stays a NaN, as in torch.clamp (fminf / fmaxf drop it)
  }
}


// ------------------------------------------------------------------------------------ LSTM
// AlignmentModule's bidirectional nn.LSTM (model/alignment_module.py:24-30), batch-major.
// The input projection, the per-step recurrent product h W_hh^T (+ b_hh + the projection
// row, as GEMM epilogue) and all weight / input gradients are sca_gemm launches; these
// two kernels are the pointwise cell of one time step, both directions in one launch
// (grid.y = direction; direction 1 walks t = T-1 .. 0).  Layouts, D = ndir:
//   gates (B, D*4H) this step's pre-activations, gate order i, f, g, o (torch's)
//   act   (B, T, D*4H) saved activations      c, y (B, T, D*H) cell / hidden states
//   hp    (B, T, D*H) the hidden state each step READS: h_{t-1} (dir 0) / h_{t+1} (dir 1),
//         zero where there is none (the caller zero-fills it once)
//   dh, dc (B, D*H) scratch of the backward walk;  dg (B, T, D*4H) gate pre-activation grads
struct LstmArgs {
  const float* gates;
  float *act, *c, *y, *hp;
  const float *dh, *dy;
  float *dc, *dg;
  int B, T, H, D, step;
  const int* valid;  // VALID kernels only: frames t >= clamp(*valid >> shift, 1, T) hold zero state
  int shift;
};

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// VALID: a step whose frame t >= nv writes c = y = 0, zero activations and a zero hp for the
// next frame, so direction 1 reaches t = nv-1 with zero state — step 0 of an unpadded run.
template <bool VALID>
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(LstmArgs a) {
  const int dir = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * a.H) return;
  const int b = idx / a.H, j = idx - b * a.H, H = a.H, DH = a.D * H;
  const int t = dir ? a.T - 1 - a.step : a.step;
  const int tp = dir ? t + 1 : t - 1, tn = dir ? t - 1 : t + 1;
  const long row = (long)b * a.T + t;
  if (VALID && t >= valid_len(a.valid, a.shift, a.T)) {
    a.c[row * DH + dir * H + j] = 0.0f;
    a.y[row * DH + dir * H + j] = 0.0f;
    if (tn >= 0 && tn < a.T) a.hp[((long)b * a.T + tn) * DH + dir * H + j] = 0.0f;
    float* az = a.act + row * 4 * DH + dir * 4 * H;
    az[j] = 0.0f; az[H + j] = 0.0f; az[2 * H + j] = 0.0f; az[3 * H + j] = 0.0f;
    return;
  }
  const float* g = a.gates + (long)b * 4 * DH + dir * 4 * H;
  const float gi = sigm(g[j]), gf = sigm(g[H + j]), gg = tanhf(g[2 * H + j]), go = sigm(g[3 * H + j]);
  const float cp = (tp >= 0 && tp < a.T) ? a.c[((long)b * a.T + tp) * DH + dir * H + j] : 0.0f;
  const float c = gf * cp + gi * gg;
  const float h = go * tanhf(c);
  a.c[row * DH + dir * H + j] = c;
  a.y[row * DH + dir * H + j] = h;
  if (tn >= 0 && tn < a.T) a.hp[((long)b * a.T + tn) * DH + dir * H + j] = h;
  float* ac = a.act + row * 4 * DH + dir * 4 * H;
  ac[j] = gi; ac[H + j] = gf; ac[2 * H + j] = gg; ac[3 * H + j] = go;
}

// backward step `step` walks t = T-1-step (dir 0) / t = step (dir 1); dh holds
// dY_t + dG_{t'} W_hh (GEMM with the dY row as residual) except at step 0, where it is dY_t
// VALID: a frame t >= nv writes dg = 0 and dc = 0 whatever dh holds; the step at t = nv-1 then
// sees dh = dY_t + 0 W_hh and dc = 0, the unpadded run's step 0.
template <bool VALID>
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(LstmArgs a) {
  const int dir = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * a.H) return;
  const int b = idx / a.H, j = idx - b * a.H, H = a.H, DH = a.D * H;
  const int t = dir ? a.step : a.T - 1 - a.step;
  const int tp = dir ? t + 1 : t - 1;
  const long row = (long)b * a.T + t;
  if (VALID && t >= valid_len(a.valid, a.shift, a.T)) {
    float* dz = a.dg + row * 4 * DH + dir * 4 * H;
    dz[j] = 0.0f; dz[H + j] = 0.0f; dz[2 * H + j] = 0.0f; dz[3 * H + j] = 0.0f;
    a.dc[(long)b * DH + dir * H + j] = 0.0f;
    return;
  }
  const float dh = a.step == 0 ? a.dy[row * DH + dir * H + j] : a.dh[(long)b * DH + dir * H + j];
  const float dcn = a.step == 0 ? 0.0f : a.dc[(long)b * DH + dir * H + j];
  const float* ac = a.act + row * 4 * DH + dir * 4 * H;
  const float gi = ac[j], gf = ac[H + j], gg = ac[2 * H + j], go = ac[3 * H + j];
  const float tc = tanhf(a.c[row * DH + dir * H + j]);
  const float cp = (tp >= 0 && tp < a.T) ? a.c[((long)b * a.T + tp) * DH + dir * H + j] : 0.0f;
  const float dcc = dcn + dh * go * (1.0f - tc * tc);
  float* dg = a.dg + row * 4 * DH + dir * 4 * H;
  dg[j] = dcc * gg * gi * (1.0f - gi);
  dg[H + j] = dcc * cp * gf * (1.0f - gf);
  dg[2 * H + j] = dcc * gi * (1.0f - gg * gg);
  dg[3 * H + j] = dh * tc * go * (1.0f - go);
  a.dc[(long)b * DH + dir * H + j] = dcc * gf;
}

bool ctc_dims_ok(int B, int T, int C, int S) {
  return B >= 1 && T >= 1 && C >= 1 && C <= SCA_CTC_MAX_C && S >= 1 && S <= SCA_CTC_MAX_S;
}

}  // namespace

// the row max / log-sum-exp pass of one tensor (ctc.h)
void sca_ctc_rowstat_launch(const float* x, float* rowstat, long rows, int C, hipStream_t st) {
  hipLaunchKernelGGL(ctc_rowstat_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, rowstat, rows, C);
}

extern "C" long sca_ctc_workspace_floats(int B, int T, int S) {
  const long BT = (long)B * T;
  return 2 * BT + 2 * BT * (2L * S + 1) + 2L * B;
}

extern "C" int sca_ctc_loss_fwd(const float* logits, const int* labels, const int* in_len, const int* tgt_len, int B,
                                int T, int C, int S, float* nll, float* loss, float* ws, void* stream) {
  if (!ctc_dims_ok(B, T, C, S) || !logits || !labels || !in_len || !tgt_len || !loss || !ws) {
    sca_set_error("sca_ctc_loss_fwd: bad arguments (C <= 8192, 1 <= S <= 1023)");
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const CtcDims d{B, T, C, S};
  const long rows = (long)B * T;
  sca_ctc_rowstat_launch(logits, ws, rows, C, st);
  hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3(B, 2), dim3(CTC_THREADS), 0, st, logits, labels, in_len, tgt_len,
                     d, ws);
  hipLaunchKernelGGL(ctc_finalize_kernel, dim3(1), dim3(256), 0, st, d, ws, nll, loss);
  return sca_launch_status("sca_ctc_loss_fwd");
}

extern "C" int sca_ctc_loss_bwd(const float* logits, const int* labels, const int* in_len, const int* tgt_len, int B,
                                int T, int C, int S, const float* dloss, const float* ws, float* dlogits,
                                void* stream) {
  if (!ctc_dims_ok(B, T, C, S) || !logits || !labels || !in_len || !tgt_len || !dloss || !ws || !dlogits) {
    sca_set_error("sca_ctc_loss_bwd: bad arguments (C <= 8192, 1 <= S <= 1023)");
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3(T, B), dim3(CTC_THREADS), 0, st, logits, labels, in_len, tgt_len,
                     CtcDims{B, T, C, S}, ws, dloss, dlogits);
  return sca_launch_status("sca_ctc_loss_bwd");
}

extern "C" long sca_seqkd_workspace_floats(int R) { return 5L * R + 1; }

namespace {

bool valid_args_ok(int T, const int* valid, int shift) { return T >= 1 && valid && shift >= 0 && shift <= 30; }

int bad_arguments(const char* name) {
  char msg[128];
  snprintf(msg, sizeof(msg), "%s: bad arguments", name);
  sca_set_error(msg);
  return SCA_ERR_ARG;
}

template <bool VALID>
int seqkd_fwd(const float* student, const float* teacher, int R, int C, int start, float temp, float weight,
              float lo, float hi, float* loss, float* ws, int T, const int* valid, int shift, void* stream,
              const char* name) {
  if (R < 1 || C < 1 || start < 0 || start >= C || !(temp > 0.0f) || !student || !teacher || !loss || !ws ||
      (VALID && (!valid_args_ok(T, valid, shift) || R % T != 0))) {
    return bad_arguments(name);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const KdArgs a{student, teacher, R, C, start, 1.0f / temp, weight * temp * temp, lo, hi, T, valid, shift};
  hipLaunchKernelGGL(kd_row_kernel<VALID>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, a, ws);
  hipLaunchKernelGGL(kd_finalize_kernel<VALID>, dim3(1), dim3(256), 0, st, a, ws, loss);
  return sca_launch_status(name);
}

template <bool VALID>
int seqkd_bwd(const float* student, const float* teacher, int R, int C, int start, float temp, const float* dloss,
              const float* ws, float* dstudent, float* dteacher, int T, const int* valid, int shift, void* stream,
              const char* name) {
  if (R < 1 || C < 1 || start < 0 || start >= C || !(temp > 0.0f) || !student || !teacher || !dloss || !ws ||
      (!dstudent && !dteacher) || (VALID && (!valid_args_ok(T, valid, shift) || R % T != 0))) {
    return bad_arguments(name);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const KdArgs a{student, teacher, R, C, start, 1.0f / temp, 0.0f, 0.0f, 0.0f, T, valid, shift};
  hipLaunchKernelGGL(kd_grad_kernel<VALID>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, a, ws, dloss, dstudent,
                     dteacher);
  return sca_launch_status(name);
}

template <bool VALID>
int lstm_cell_fwd(const float* gates, float* act, float* c, float* y, float* hp, int B, int T, int H, int ndir,
                  int step, const int* valid, int shift, void* stream, const char* name) {
  if (B < 1 || T < 1 || H < 1 || ndir < 1 || ndir > 2 || step < 0 || step >= T || !gates || !act || !c || !y ||
      !hp || (VALID && !valid_args_ok(T, valid, shift))) {
    return bad_arguments(name);
  }
  LstmArgs a{gates, act, c, y, hp, nullptr, nullptr, nullptr, nullptr, B, T, H, ndir, step, valid, shift};
  hipLaunchKernelGGL(lstm_cell_fwd_kernel<VALID>, dim3((B * H + 255) / 256, ndir), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return sca_launch_status(name);
}

template <bool VALID>
int lstm_cell_bwd(const float* dh, const float* dy, const float* act, const float* c, float* dc, float* dg, int B,
                  int T, int H, int ndir, int step, const int* valid, int shift, void* stream, const char* name) {
  if (B < 1 || T < 1 || H < 1 || ndir < 1 || ndir > 2 || step < 0 || step >= T || !dy || !act || !c || !dc ||
      !dg || (step > 0 && !dh) || (VALID && !valid_args_ok(T, valid, shift))) {
    return bad_arguments(name);
  }
  LstmArgs a{nullptr, const_cast<float*>(act), const_cast<float*>(c), nullptr, nullptr, dh, dy, dc, dg,
             B, T, H, ndir, step, valid, shift};
  hipLaunchKernelGGL(lstm_cell_bwd_kernel<VALID>, dim3((B * H + 255) / 256, ndir), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return sca_launch_status(name);
}

}  // namespace

extern "C" int sca_seqkd_fwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                             float weight, float lo, float hi, float* loss, float* ws, void* stream) {
  return seqkd_fwd<false>(student, teacher, R, C, start, temp, weight, lo, hi, loss, ws, 1, nullptr, 0, stream,
                          "sca_seqkd_fwd");
}

extern "C" int sca_seqkd_valid_fwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                                   float weight, float lo, float hi, float* loss, float* ws, int T,
                                   const int* valid_frames, int shift, void* stream) {
  return seqkd_fwd<true>(student, teacher, R, C, start, temp, weight, lo, hi, loss, ws, T, valid_frames, shift,
                         stream, "sca_seqkd_valid_fwd");
}

extern "C" int sca_seqkd_bwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                             const float* dloss, const float* ws, float* dstudent, float* dteacher, void* stream) {
  return seqkd_bwd<false>(student, teacher, R, C, start, temp, dloss, ws, dstudent, dteacher, 1, nullptr, 0, stream,
                          "sca_seqkd_bwd");
}

extern "C" int sca_seqkd_valid_bwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                                   const float* dloss, const float* ws, float* dstudent, float* dteacher, int T,
                                   const int* valid_frames, int shift, void* stream) {
  return seqkd_bwd<true>(student, teacher, R, C, start, temp, dloss, ws, dstudent, dteacher, T, valid_frames, shift,
                         stream, "sca_seqkd_valid_bwd");
}

extern "C" int sca_clamp(const float* x, float* y, const float* dy, float* dx, long n, float lo, float hi,
                         void* stream) {
  if (n < 0 || !x || (dy ? !dx : !y)) {
    sca_set_error("sca_clamp: bad arguments");
    return SCA_ERR_ARG;
  }
  if (n == 0) return SCA_OK;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(clamp_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, y, dy, dx, n, lo, hi);
  return sca_launch_status("sca_clamp");
}

extern "C" int sca_lstm_cell_fwd(const float* gates, float* act, float* c, float* y, float* hp, int B, int T, int H,
                                 int ndir, int step, void* stream) {
  return lstm_cell_fwd<false>(gates, act, c, y, hp, B, T, H, ndir, step, nullptr, 0, stream, "sca_lstm_cell_fwd");
}

extern "C" int sca_lstm_cell_valid_fwd(const float* gates, float* act, float* c, float* y, float* hp, int B, int T,
                                       int H, int ndir, int step, const int* valid_frames, int shift, void* stream) {
  return lstm_cell_fwd<true>(gates, act, c, y, hp, B, T, H, ndir, step, valid_frames, shift, stream,
                             "sca_lstm_cell_valid_fwd");
}

extern "C" int sca_lstm_cell_bwd(const float* dh, const float* dy, const float* act, const float* c, float* dc,
                                 float* dg, int B, int T, int H, int ndir, int step, void* stream) {
  return lstm_cell_bwd<false>(dh, dy, act, c, dc, dg, B, T, H, ndir, step, nullptr, 0, stream, "sca_lstm_cell_bwd");
}

extern "C" int sca_lstm_cell_valid_bwd(const float* dh, const float* dy, const float* act, const float* c, float* dc,
                                       float* dg, int B, int T, int H, int ndir, int step, const int* valid_frames,
                                       int shift, void* stream) {
  return lstm_cell_bwd<true>(dh, dy, act, c, dc, dg, B, T, H, ndir, step, valid_frames, shift, stream,
                             "sca_lstm_cell_valid_bwd");
}
