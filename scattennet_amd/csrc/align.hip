// CTC forced alignment on the device: for a (head, clip) and a label sequence, the Viterbi
// path through the 2 S + 1 extended CTC states, from which come the frame span [start, end)
// and the mean posterior of every label (gloss boundaries, sign spotting, re-alignment
// pseudo-labels), and sca_eval_log_alignments, which appends them to an evaluation pass's log
// beside the hypotheses of sca_eval_accumulate.  Semantics: include/scatten.h.
//
// A clip's T_b frames are a dependent chain (as in the beam search of decode.hip), so a
// (head, clip) is one workgroup and the recursion is latency-bound: v is ping-ponged in LDS,
// only the reachable band of states is visited, a frame costs one LDS barrier when the clip has
// more than 64 states and none when it has not (one wave, in-order LDS), and the logits a frame
// needs are asked for ALN_AHEAD frames earlier.  A back-pointer is two bits, packed by ballot
// into two 64-bit words per (frame, 64 states); they stay in LDS when they fit.  No atomics
// on floats; every sum runs in a fixed order: results are deterministic.
#include "ctc.h"

namespace {

constexpr int ALN_MAX_L = 2 * SCA_CTC_MAX_S + 1;  // 2047 extended states
constexpr int ALN_AHEAD = 4;                      // frames of logits in flight
constexpr int ALN_BP_LDS = 1024;                  // (frame, 64-state chunk) pairs of back-pointers kept in LDS
constexpr int ALN_SMALL_L = 512;                  // up to here 256 threads, above 1024: two states per thread

struct AlnDims {
  int B, T, C, S;
};

__host__ __device__ __forceinline__ int aln_chunks(int S) { return (2 * S + 1 + 63) / 64; }

// One workgroup per (clip, head): grid (B, G).  Thread tid owns the extended states tid and
// tid + NT for the whole clip (their class and whether the skip transition is allowed stay in
// registers), so a wave is one aligned chunk of 64 states and its back-pointers are two ballots.
template <int NT>
__global__ __launch_bounds__(NT) void ctc_align_kernel(CtcHeads hx, const int* __restrict__ in_len,
                                                       const int* __restrict__ labels,
                                                       const int* __restrict__ lab_len, int per_head, AlnDims d,
                                                       int* __restrict__ frame_label, int* __restrict__ spans,
                                                       float* __restrict__ conf, float* __restrict__ score,
                                                       const float* __restrict__ rowstat,
                                                       unsigned long long* __restrict__ bp_g, int bp_lds) {
  __shared__ float s_v[2][ALN_MAX_L + 1];
  __shared__ unsigned long long s_bp[2 * ALN_BP_LDS];
  __shared__ int s_start[SCA_CTC_MAX_S + 1], s_end[SCA_CTC_MAX_S + 1];
  __shared__ int s_fin;  // the path's end state, -1: nothing to walk back
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, g = blockIdx.y;
  const int slot = g * d.B + b;  // the (head, clip)'s place in the workspace and the outputs
  const int T = d.T, C = d.C, S = d.S;
  const int Tb = clampi(in_len[b], 0, T);
  const int lrow = per_head ? slot : b;
  const int Sb = clampi(lab_len[lrow], 0, S);
  const int* __restrict__ lab = labels + (long)lrow * S;
  const int L = 2 * Sb + 1, nchunk = aln_chunks(S);
  const float* __restrict__ x = ctc_head(hx, g) + (long)b * T * C;  // the clip's (T, C) logits
  const float* __restrict__ rs = rowstat + 2 * (long)slot * T;
  unsigned long long* __restrict__ bpg = bp_g + 2 * (long)slot * T * nchunk;
  int* __restrict__ fl = frame_label + (long)slot * T;

  int cls[2];
  bool skip[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s = tid + i * NT;
    cls[i] = 0;
    skip[i] = false;
    if (s < L && (s & 1)) {
      const int j = s >> 1;
      cls[i] = clampi(lab[j], 1, C - 1);
      skip[i] = j >= 1 && cls[i] != clampi(lab[j - 1], 1, C - 1);
    }
  }
  for (int i = tid; i < 2 * (ALN_MAX_L + 1); i += NT) (&s_v[0][0])[i] = NEG_INF;
  for (int j = tid; j < S; j += NT) {
    s_start[j] = 0;
    s_end[j] = 0;
  }
  __syncthreads();

  const bool solo = L <= 64;  // one wave holds every state: no workgroup barrier in the chain
  if (!solo || wave == 0) {
    float xq[ALN_AHEAD][2], mq[ALN_AHEAD], lq[ALN_AHEAD];
    auto fetch = [&](int t, float (&xv)[2], float& m, float& ls) {
      m = rs[2 * t];
      ls = rs[2 * t + 1];
#pragma unroll
      for (int i = 0; i < 2; ++i) xv[i] = tid + i * NT < L ? x[(long)t * C + cls[i]] : 0.0f;
    };
#pragma unroll
    for (int dd = 0; dd < ALN_AHEAD; ++dd) {
      mq[dd] = lq[dd] = xq[dd][0] = xq[dd][1] = 0.0f;
      if (dd < Tb) fetch(dd, xq[dd], mq[dd], lq[dd]);
    }
    for (int t0 = 0; t0 < Tb; t0 += ALN_AHEAD) {
#pragma unroll
      for (int dd = 0; dd < ALN_AHEAD; ++dd) {
        const int t = t0 + dd;
        if (t < Tb) {  // uniform
          const float xv[2] = {xq[dd][0], xq[dd][1]};
          const float m = mq[dd], ls = lq[dd];
          if (t + ALN_AHEAD < Tb) fetch(t + ALN_AHEAD, xq[dd], mq[dd], lq[dd]);
          // the states that are reachable from the start and can still reach the end
          const int lo = max(0, L - 2 * (Tb - t)), hi = min(L - 1, 2 * t + 1);
          const int cur = t & 1, prev = cur ^ 1;
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int cs = (tid & ~63) + i * NT;  // the wave's chunk of states
            if (cs <= hi && cs + 63 >= lo) {      // wave-uniform
              const int s = tid + i * NT;
              const bool in = s >= lo && s <= hi;
              float a = NEG_INF, b1 = NEG_INF, c2 = NEG_INF;
              if (in) {
                if (t == 0) {
                  a = s <= 1 ? 0.0f : NEG_INF;
                } else {
                  a = s_v[prev][s];
                  if (s >= 1) b1 = s_v[prev][s - 1];
                  if (skip[i]) c2 = s_v[prev][s - 2];
                }
              }
              // ties: stay in s unless s - 1 is strictly greater; s - 2 only if greater than both
              float best = a;
              int k = 0;
              if (b1 > best) { best = b1; k = 1; }
              if (c2 > best) { best = c2; k = 2; }
              if (in) s_v[cur][s] = ctc_lp_raw(xv[i], m, ls) + best;
              if (t > 0) {
                const unsigned long long k0 = __ballot(k & 1), k1 = __ballot(k >> 1);
                if (lane == 0) {
                  const long idx = 2 * ((long)t * nchunk + (cs >> 6));
                  if (bp_lds) {
                    s_bp[idx] = k0;
                    s_bp[idx + 1] = k1;
                  } else {
                    bpg[idx] = k0;
                    bpg[idx + 1] = k1;
                  }
                }
              }
            }
          }
          if (solo) wave_lds_sync();
          else lds_barrier();
        }
      }
    }
  }
  __syncthreads();

  if (tid == 0) {
    float sc;
    int e = -1;
    if (Tb == 0) {
      sc = Sb == 0 ? 0.0f : NEG_INF;
    } else {
      const int fb = (Tb - 1) & 1;
      e = L == 1 ? 0 : (s_v[fb][L - 1] > s_v[fb][L - 2] ? L - 1 : L - 2);
      sc = s_v[fb][e];
      if (sc == NEG_INF) e = -1;  // infeasible
    }
    int s = e, after = -1;  // after: the state of frame t + 1
    for (int t = e >= 0 ? Tb - 1 : -1; t >= 0; --t) {
      if (s & 1) {
        const int j = s >> 1;
        fl[t] = j;
        if (s != after) s_end[j] = t + 1;
        s_start[j] = t;
      } else {
        fl[t] = -1;
      }
      after = s;
      if (t > 0) {
        const long idx = 2 * ((long)t * nchunk + (s >> 6));
        const unsigned long long k0 = bp_lds ? s_bp[idx] : bpg[idx], k1 = bp_lds ? s_bp[idx + 1] : bpg[idx + 1];
        const int k = (int)((k0 >> (s & 63)) & 1ull) | ((int)((k1 >> (s & 63)) & 1ull) << 1);
        s = max(s - k, 0);  // k <= s on a finite path; stay in bounds whatever the logits held
      }
    }
    score[slot] = sc;
    s_fin = e;
  }
  __syncthreads();

  const bool feasible = s_fin >= 0;
  for (int t = tid; t < T; t += NT)
    if (!feasible || t >= Tb) fl[t] = -1;
  for (int j = tid; j < S; j += NT) {
    int st = 0, en = 0;
    float cv = 0.0f;
    if (feasible && j < Sb) {
      st = s_start[j];
      en = s_end[j];
      const int c = clampi(lab[j], 1, C - 1);
      float sum = 0.0f;
      for (int t = st; t < en; ++t) sum += __expf(ctc_lp_raw(x[(long)t * C + c], rs[2 * t], rs[2 * t + 1]));
      cv = en > st ? sum / (float)(en - st) : 0.0f;
    }
    spans[2 * ((long)slot * S + j)] = st;
    spans[2 * ((long)slot * S + j) + 1] = en;
    conf[(long)slot * S + j] = cv;
  }
}

// grid (B, G): clip b's alignment of head g into row cursor + b of the logs
__global__ __launch_bounds__(128) void eval_log_align_kernel(const int* __restrict__ spans,
                                                             const float* __restrict__ conf,
                                                             const float* __restrict__ score, int S,
                                                             const sca_eval_state* __restrict__ state,
                                                             int* __restrict__ span_log, float* __restrict__ conf_log,
                                                             float* __restrict__ score_log, int capacity, int width) {
  const int b = blockIdx.x, g = blockIdx.y, B = gridDim.x, G = gridDim.y, tid = threadIdx.x;
  const long row = (long)state->cursor + b;
  if (row >= capacity) return;  // sca_eval_accumulate raises SCA_EVAL_LOG_DROPPED for this clip
  const long n = (long)g * B + b, dst = row * G + g;
  for (int j = tid; j < width; j += 128) {
    const bool have = j < S;
    span_log[2 * (dst * width + j)] = have ? spans[2 * (n * S + j)] : 0;
    span_log[2 * (dst * width + j) + 1] = have ? spans[2 * (n * S + j) + 1] : 0;
    conf_log[dst * width + j] = have ? conf[n * S + j] : 0.0f;
  }
  if (tid == 0) score_log[dst] = score[n];
}

bool aln_dims_ok(int G, int B, int T, int S) {
  return G >= 1 && G <= SCA_EVAL_MAX_HEADS && B >= 1 && T >= 1 && S >= 0 && S <= SCA_CTC_MAX_S &&
         (long)G * B <= 0x7fffffffL / 4;
}

}  // namespace

extern "C" long sca_ctc_align_workspace_bytes(int G, int B, int T, int S) {
  if (!aln_dims_ok(G, B, T, S)) return 0;
  const long NT = (long)G * B * T;  // row statistics, then the back-pointers of every (head, clip)
  return 4 * 2 * NT + 8 * 2 * NT * aln_chunks(S);
}

extern "C" int sca_ctc_align_heads(const sca_decode_heads* heads, int G, const int* in_len, const int* labels,
                                   const int* lab_len, int labels_per_head, int B, int T, int C, int S,
                                   int* frame_label, int* spans, float* conf, float* score, void* ws, void* stream) {
  bool ok = aln_dims_ok(G, B, T, S) && C >= 1 && C <= SCA_CTC_MAX_C && heads && in_len && lab_len && frame_label &&
            score && ws && (S == 0 || (labels && spans && conf));
  for (int g = 0; ok && g < G; ++g) ok = heads->logits[g] != nullptr;
  if (!ok) {
    sca_set_error("sca_ctc_align_heads: bad arguments (1 <= G <= 8 non-null tensors, B, T >= 1, 1 <= C <= 8192, "
                  "0 <= S <= 1023)");
    return SCA_ERR_ARG;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const AlnDims d{B, T, C, S};
  const CtcHeads hx = ctc_heads_of(heads, G);
  float* rowstat = static_cast<float*>(ws);
  const long NT = (long)G * B * T;
  unsigned long long* bp = reinterpret_cast<unsigned long long*>(rowstat + 2 * NT);  // 8 NT bytes in front
  const int bp_lds = (long)T * aln_chunks(S) <= ALN_BP_LDS;
  sca_ctc_rowstat_heads_launch(heads, G, rowstat, (long)B * T, C, st);
  if (2 * S + 1 <= ALN_SMALL_L)
    hipLaunchKernelGGL(ctc_align_kernel<256>, dim3(B, G), dim3(256), 0, st, hx, in_len, labels, lab_len,
                       labels_per_head != 0, d, frame_label, spans, conf, score, rowstat, bp, bp_lds);
  else
    hipLaunchKernelGGL(ctc_align_kernel<1024>, dim3(B, G), dim3(1024), 0, st, hx, in_len, labels, lab_len,
                       labels_per_head != 0, d, frame_label, spans, conf, score, rowstat, bp, bp_lds);
  return sca_launch_status("sca_ctc_align_heads");
}

extern "C" int sca_eval_log_alignments(const int* spans, const float* conf, const float* score, int G, int B, int S,
                                       const sca_eval_state* state, int* span_log, float* conf_log, float* score_log,
                                       int capacity, int log_width, void* stream) {
  if (G < 1 || G > SCA_EVAL_MAX_HEADS || B < 1 || S < 0 || capacity < 1 || log_width < 1 || !score || !state ||
      !span_log || !conf_log || !score_log || (S > 0 && (!spans || !conf))) {
    sca_set_error("sca_eval_log_alignments: bad arguments (1 <= G <= 8, B >= 1, S >= 0, capacity, log_width >= 1)");
    return SCA_ERR_ARG;
  }
  hipLaunchKernelGGL(eval_log_align_kernel, dim3(B, G), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), spans,
                     conf, score, S, state, span_log, conf_log, score_log, capacity, log_width);
  return sca_launch_status("sca_eval_log_alignments");
}
