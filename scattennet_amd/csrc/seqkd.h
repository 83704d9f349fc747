// The SeqKD row arithmetic (loss.py:5-21 with the weight and clamp of model/__init__.py:203-214),
// one body under heads.hip (sca_seqkd_*, one student and one teacher tensor per call) and
// distill.hip (sca_distill_heads_*, several students per launch), so that the grouped call with one
// member is bitwise the single call per student.
#pragma once
#include "ctc.h"

struct KdArgs {
  const float *s, *q;
  int R, C, start;
  float inv_temp, weight_t2, lo, hi;
  int T;             // VALID kernels only: rows are (b, t), t = row % T, and only t < nv take part,
  const int* valid;  // nv = clamp(*valid >> shift, 1, T) read on the device
  int shift;
};

// the valid length of the *_valid entry points: a device scalar (a graph replay sees what the
// host last copied there), clamped so a bad value stays in bounds
__device__ __forceinline__ int valid_len(const int* valid, int shift, int T) {
  const int nv = *valid >> shift;
  return nv < 1 ? 1 : (nv > T ? T : nv);
}

// ws layout: row_loss[R] | stats[4R] (student max, log-sum, teacher max, log-sum) | dscale[1]
// VALID: a row with t >= nv leaves a zero row loss (the fixed-order sum of the finalize step
// then adds exact zeros) and zero statistics.
// One row by one wave.
template <bool VALID>
__device__ __forceinline__ void kd_row(const KdArgs& a, float* ws, long row, int lane) {
  if (VALID && (int)(row % a.T) >= valid_len(a.valid, a.shift, a.T)) {
    if (lane == 0) {
      ws[row] = 0.0f;
      float* st = ws + a.R + 4 * row;
      st[0] = 0.0f; st[1] = 0.0f; st[2] = 0.0f; st[3] = 0.0f;
    }
    return;
  }
  const float* sr = a.s + row * a.C;
  const float* qr = a.q + row * a.C;
  float ms = NEG_INF, mq = NEG_INF;
  for (int c = a.start + lane; c < a.C; c += 64) {
    ms = fmaxf(ms, sr[c] * a.inv_temp);
    mq = fmaxf(mq, qr[c] * a.inv_temp);
  }
  ms = wave_max(ms);
  mq = wave_max(mq);
  float ss = 0.0f, sq = 0.0f;
  for (int c = a.start + lane; c < a.C; c += 64) {
    ss += __expf(sr[c] * a.inv_temp - ms);
    sq += __expf(qr[c] * a.inv_temp - mq);
  }
  const float lss = __logf(wave_sum(ss));
  const float sq_all = wave_sum(sq);
  const float lsq = __logf(sq_all);
  // KLDivLoss (log_target=False): xlogy(p, p) - p * log_softmax(student)
  float acc = 0.0f;
  for (int c = a.start + lane; c < a.C; c += 64) {
    const float p = __expf(qr[c] * a.inv_temp - mq) / sq_all;  // F.softmax
    const float lsm = (sr[c] * a.inv_temp - ms) - lss;         // F.log_softmax
    acc += (p > 0.0f ? p * __logf(p) : 0.0f) - p * lsm;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    ws[row] = acc;
    float* st = ws + a.R + 4 * row;
    st[0] = ms; st[1] = lss; st[2] = mq; st[3] = lsq;
  }
}

// One workgroup of 256 threads: the loss of one (student, teacher) pair from its row losses, and
// the clamp gate with the scale of the backward in ws[5R].  red: 4 floats of LDS.
template <bool VALID>
__device__ __forceinline__ void kd_finalize(const KdArgs& a, float* ws, float* loss, float* red, int tid) {
  float s = 0.0f;
  for (int r = tid; r < a.R; r += 256) s += ws[r];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    // batchmean over the R = B*T rows of the .view(-1, C') (loss.py:13-19), * T^2 * weight;
    // VALID: over the B*nv rows that took part
    const float rows = VALID ? (float)((a.R / a.T) * valid_len(a.valid, a.shift, a.T)) : (float)a.R;
    const float v = (red[0] + red[1] + red[2] + red[3]) / rows * a.weight_t2;
    loss[0] = fminf(fmaxf(v, a.lo), a.hi);
    ws[5L * a.R] = (v >= a.lo && v <= a.hi) ? a.weight_t2 / rows : 0.0f;
  }
}

// One row by one wave: d loss / d student (ds) and / d teacher (dq), either may be null.
template <bool VALID>
__device__ __forceinline__ void kd_grad_row(const KdArgs& a, const float* ws, const float* dloss, float* ds, float* dq,
                                            long row, int lane) {
  if (VALID && (int)(row % a.T) >= valid_len(a.valid, a.shift, a.T)) {  // exact zeros behind the valid frames
    for (int c = lane; c < a.C; c += 64) {
      if (ds) ds[row * a.C + c] = 0.0f;
      if (dq) dq[row * a.C + c] = 0.0f;
    }
    return;
  }
  const float k = dloss[0] * ws[5L * a.R] * a.inv_temp;
  const float* st = ws + a.R + 4 * row;
  const float ms = st[0], lss = st[1], mq = st[2], lsq = st[3];
  const float* sr = a.s + row * a.C;
  const float* qr = a.q + row * a.C;
  float hbar = 0.0f;
  if (dq) {  // sum_c p_c (log p_c - log_softmax(student)_c) for the teacher's softmax backward
    for (int c = a.start + lane; c < a.C; c += 64) {
      const float lp = (qr[c] * a.inv_temp - mq) - lsq;
      hbar += __expf(lp) * (lp - ((sr[c] * a.inv_temp - ms) - lss));
    }
    hbar = wave_sum(hbar);
  }
  for (int c = lane; c < a.C; c += 64) {
    float gs = 0.0f, gq = 0.0f;
    if (c >= a.start) {
      const float lsm = (sr[c] * a.inv_temp - ms) - lss;
      const float lp = (qr[c] * a.inv_temp - mq) - lsq;
      const float p = __expf(lp);
      gs = k * (__expf(lsm) - p);
      gq = k * p * ((lp - lsm) - hbar);
    }
    if (ds) ds[row * a.C + c] = gs;
    if (dq) dq[row * a.C + c] = gq;
  }
}
